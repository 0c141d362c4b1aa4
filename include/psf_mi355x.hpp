// psf_mi355x.hpp -- C++ host-side mirror of the reference's `PSF` trait (src/primitive/psf.rs:39-81) over the C ABI of
// psf_mi355x.h.  Header-only; link with -lpsf_mi355x.  The reference is Rust; no Rust toolchain exists in the build image,
// so this is the compiled-language face of the drop-in (INTEGRATION.md shows the equivalent Rust shim).
//
//   trait PSF { type A; type Trapdoor; type Domain; type Range;
//               fn trap_gen(&self) -> (A, Trapdoor);  fn samp_d(&self) -> Domain;
//               fn samp_p(&self, a, r, u) -> Domain;   fn f_a(&self, a, sigma) -> Range;  fn check_domain(&self, sigma) -> bool; }
//
// Differences that the ABI imposes and this mirror keeps explicit:
//   * randomness is seeded (the trait has no seed, psf.rs:48-80): every sampling method takes (seed, first_index);
//   * a call may carry B rows (B independent reference calls); vectors are flat row-major std::vector;
//   * the key lives in the handle (device memory): samp_p / f_a use the key of the last trap_gen / load_key, so the
//     `a` and `r` arguments of the trait are implicit;
//   * where the reference panics, PsfError is thrown.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>
#include "psf_mi355x.h"

namespace psf_mi355x {

struct PsfError : std::runtime_error {
  psf_status status;
  PsfError(psf_status s, const char* where) : std::runtime_error(std::string(where) + ": " + psf_status_string(s)), status(s) {}
};
inline void check(psf_status s, const char* where) { if (s != PSF_OK) throw PsfError(s, where); }

// GadgetParameters::init_default (gadget_parameters.rs:113-133) / GadgetParametersRing::init_default (:165-185)
inline psf_gadget_params gadget_parameters_default(uint64_t n, uint64_t q) {
  psf_gadget_params gp;
  check(psf_gadget_params_default(n, q, &gp), "GadgetParameters::init_default");
  return gp;
}
inline psf_gadget_params gadget_parameters_ring_default(uint64_t n, uint64_t q) {
  psf_gadget_params gp;
  check(psf_gadget_params_ring_default(n, q, &gp), "GadgetParametersRing::init_default");
  return gp;
}

using MatZq = std::vector<uint64_t>;   // least non-negative residues, row-major
using MatZ = std::vector<int64_t>;

// ---- fused R_q matrix products C[c] = E[c] + sign * op(A[c]) B[c] on device buffers (psf_matpoly_mul_add_*_dev; layouts and rules in psf_mi355x.h) ----
// d_e == d_c accumulates in place.  `cyclic`: Z_q[X]/(X^n - 1) instead of Z_q[X]/(X^n + 1).
struct MatPolyShape { size_t count, rows, inner, cols; int trans_a = 0; };
inline void matpoly_mul_add_dev(int device, uint64_t q, size_t n, const MatPolyShape& s, const void* d_a, size_t a_stride, const void* d_b, const void* d_e, int sign,
                                void* d_c, int io_bits = 64, void* stream = nullptr, bool cyclic = false) {
  check((cyclic ? psf_matpoly_mul_add_cyclic_dev : psf_matpoly_mul_add_negacyclic_dev)(device, q, n, s.count, s.rows, s.inner, s.cols, d_a, a_stride, s.trans_a, d_b,
                                                                                      d_e, sign, d_c, io_bits, stream), "matpoly_mul_add_dev");
}
inline void matpoly_mul_add_hat_dev(int device, uint64_t q, size_t n, const MatPolyShape& s, const uint32_t* d_hat, size_t hat_stride, const void* d_b, const void* d_e,
                                    int sign, void* d_c, int io_bits = 64, void* stream = nullptr, bool cyclic = false) {
  check((cyclic ? psf_matpoly_mul_add_hat_cyclic_dev : psf_matpoly_mul_add_hat_dev)(device, q, n, s.count, s.rows, s.inner, s.cols, d_hat, hat_stride, s.trans_a, d_b,
                                                                                   d_e, sign, d_c, io_bits, stream), "matpoly_mul_add_hat_dev");
}
// host buffers, one batch: a rows x inner, b inner x cols, e rows x cols polynomials of n coefficients; returns e + sign * a b in [0, q)
inline MatZq matpoly_mul_add(int device, uint64_t q, size_t n, size_t rows, size_t inner, size_t cols, const MatZq& a, const MatZ& b, const MatZ& e, int sign = 1,
                             bool cyclic = false) {
  if (a.size() != rows * inner * n || b.size() != inner * cols * n || e.size() != rows * cols * n) throw PsfError(PSF_ERR_PARAM, "matpoly_mul_add");
  MatZq c(rows * cols * n);
  check((cyclic ? psf_matpoly_mul_add_cyclic : psf_matpoly_mul_add_negacyclic)(device, q, n, rows, inner, cols, a.data(), b.data(), e.data(), sign, c.data()),
        "matpoly_mul_add");
  return c;
}

// ---- FIPS 202 / FIPS 203 on device buffers (psf_keccak_dev, psf_sample_*_fips203_dev, psf_ntt_image_*_fips203_dev; rules in psf_mi355x.h) ----------
inline void keccak_dev(int device, int func, size_t count, const uint8_t* d_in, size_t in_len, size_t in_stride, uint8_t* d_out, size_t out_len, size_t out_stride,
                       void* stream = nullptr) {
  check(psf_keccak_dev(device, func, count, d_in, in_len, in_stride, d_out, out_len, out_stride, stream), "keccak_dev");
}
// `count` messages of in_len bytes, packed; returns their digests of out_len bytes, packed
inline std::vector<uint8_t> keccak(int device, int func, size_t count, const std::vector<uint8_t>& in, size_t in_len, size_t out_len) {
  if (in.size() != count * in_len) throw PsfError(PSF_ERR_PARAM, "keccak");
  std::vector<uint8_t> out(count * out_len);
  check(psf_keccak(device, func, count, in.data(), in_len, in_len, out.data(), out_len, out_len), "keccak");
  return out;
}
// SHA-256 / SHA-512 (psf_sha2_dev, psf_sha2): func is PSF_SHA2_256 or PSF_SHA2_512, out_len the leading bytes of the digest
inline void sha2_dev(int device, int func, size_t count, const uint8_t* d_in, size_t in_len, size_t in_stride, uint8_t* d_out, size_t out_len, size_t out_stride,
                     void* stream = nullptr) {
  check(psf_sha2_dev(device, func, count, d_in, in_len, in_stride, d_out, out_len, out_stride, stream), "sha2_dev");
}
inline std::vector<uint8_t> sha2(int device, int func, size_t count, const std::vector<uint8_t>& in, size_t in_len, size_t out_len) {
  if (in.size() != count * in_len) throw PsfError(PSF_ERR_PARAM, "sha2");
  std::vector<uint8_t> out(count * out_len);
  check(psf_sha2(device, func, count, in.data(), in_len, in_len, out.data(), out_len, out_len), "sha2");
  return out;
}
// SampleNTT: k = 0 raw form (34-byte inputs), 1 <= k <= 16 matrix form (32-byte rho, count k k polynomials)
inline void sample_ntt_fips203_dev(int device, size_t count, uint32_t k, const uint8_t* d_seed, size_t seed_stride, void* d_out, int* d_fail = nullptr, int io_bits = 64,
                                   void* stream = nullptr) {
  check(psf_sample_ntt_fips203_dev(device, count, k, d_seed, seed_stride, d_out, d_fail, io_bits, stream), "sample_ntt_fips203_dev");
}
// SamplePolyCBD_eta(PRF_eta(sigma_c, first_nonce + t)), t < per_seed
inline void sample_cbd_fips203_dev(int device, size_t count, uint32_t eta, const uint8_t* d_sigma, size_t sigma_stride, uint32_t first_nonce, uint32_t per_seed, void* d_out,
                                   int io_bits = 64, void* stream = nullptr) {
  check(psf_sample_cbd_fips203_dev(device, count, eta, d_sigma, sigma_stride, first_nonce, per_seed, d_out, io_bits, stream), "sample_cbd_fips203_dev");
}
inline void ntt_image_from_fips203_dev(int device, size_t count, const void* d_fhat, uint32_t* d_hat, int io_bits = 64, void* stream = nullptr) {
  check(psf_ntt_image_from_fips203_dev(device, count, d_fhat, io_bits, d_hat, stream), "ntt_image_from_fips203_dev");
}
inline void ntt_image_to_fips203_dev(int device, size_t count, const uint32_t* d_hat, void* d_fhat, int io_bits = 64, void* stream = nullptr) {
  check(psf_ntt_image_to_fips203_dev(device, count, d_hat, d_fhat, io_bits, stream), "ntt_image_to_fips203_dev");
}

// ---- ML-KEM, batched (psf_mlkem_*; sizes, the workspace and the rules in psf_mi355x.h).  `param` is PSF_MLKEM_512 / _768 / _1024 --------------------
struct MlKemSizes { size_t ek, dk, ct, ss; };
inline MlKemSizes mlkem_sizes(int param) {
  MlKemSizes s{};
  check(psf_mlkem_sizes(param, &s.ek, &s.dk, &s.ct, &s.ss), "mlkem_sizes");
  return s;
}
inline size_t mlkem_workspace_bytes(int param, size_t count, int op) {
  size_t bytes = 0;
  check(psf_mlkem_workspace_bytes(param, count, op, &bytes), "mlkem_workspace_bytes");
  return bytes;
}
inline void mlkem_keygen_dev(int device, int param, size_t count, const uint8_t* d_d, const uint8_t* d_z, uint8_t* d_ek, uint8_t* d_dk, void* d_ws, size_t ws_bytes,
                             int* d_fail = nullptr, void* stream = nullptr) {
  check(psf_mlkem_keygen_dev(device, param, count, d_d, d_z, d_ek, d_dk, d_ws, ws_bytes, d_fail, stream), "mlkem_keygen_dev");
}
inline void mlkem_encaps_dev(int device, int param, size_t count, const uint8_t* d_ek, const uint8_t* d_m, uint8_t* d_ss, uint8_t* d_ct, void* d_ws, size_t ws_bytes,
                             int* d_fail = nullptr, void* stream = nullptr) {
  check(psf_mlkem_encaps_dev(device, param, count, d_ek, d_m, d_ss, d_ct, d_ws, ws_bytes, d_fail, stream), "mlkem_encaps_dev");
}
inline void mlkem_decaps_dev(int device, int param, size_t count, const uint8_t* d_dk, const uint8_t* d_ct, uint8_t* d_ss, void* d_ws, size_t ws_bytes,
                             int* d_fail = nullptr, void* stream = nullptr) {
  check(psf_mlkem_decaps_dev(device, param, count, d_dk, d_ct, d_ss, d_ws, ws_bytes, d_fail, stream), "mlkem_decaps_dev");
}
inline void mlkem_check_ek_dev(int device, int param, size_t count, const uint8_t* d_ek, uint8_t* d_ok, void* stream = nullptr) {
  check(psf_mlkem_check_ek_dev(device, param, count, d_ek, d_ok, stream), "mlkem_check_ek_dev");
}
inline void mlkem_check_dk_dev(int device, int param, size_t count, const uint8_t* d_dk, uint8_t* d_ok, void* stream = nullptr) {
  check(psf_mlkem_check_dk_dev(device, param, count, d_dk, d_ok, stream), "mlkem_check_dk_dev");
}
// host buffers, packed: d and z 32 bytes per instance; returns (ek, dk)
inline std::pair<std::vector<uint8_t>, std::vector<uint8_t>> mlkem_keygen(int device, int param, size_t count, const std::vector<uint8_t>& d, const std::vector<uint8_t>& z) {
  const MlKemSizes s = mlkem_sizes(param);
  if (d.size() != count * 32 || z.size() != count * 32) throw PsfError(PSF_ERR_PARAM, "mlkem_keygen");
  std::vector<uint8_t> ek(count * s.ek), dk(count * s.dk);
  check(psf_mlkem_keygen(device, param, count, d.data(), z.data(), ek.data(), dk.data()), "mlkem_keygen");
  return {ek, dk};
}
// returns (shared secrets, ciphertexts)
inline std::pair<std::vector<uint8_t>, std::vector<uint8_t>> mlkem_encaps(int device, int param, size_t count, const std::vector<uint8_t>& ek, const std::vector<uint8_t>& m) {
  const MlKemSizes s = mlkem_sizes(param);
  if (ek.size() != count * s.ek || m.size() != count * 32) throw PsfError(PSF_ERR_PARAM, "mlkem_encaps");
  std::vector<uint8_t> ss(count * s.ss), ct(count * s.ct);
  check(psf_mlkem_encaps(device, param, count, ek.data(), m.data(), ss.data(), ct.data()), "mlkem_encaps");
  return {ss, ct};
}
inline std::vector<uint8_t> mlkem_decaps(int device, int param, size_t count, const std::vector<uint8_t>& dk, const std::vector<uint8_t>& ct) {
  const MlKemSizes s = mlkem_sizes(param);
  if (dk.size() != count * s.dk || ct.size() != count * s.ct) throw PsfError(PSF_ERR_PARAM, "mlkem_decaps");
  std::vector<uint8_t> ss(count * s.ss);
  check(psf_mlkem_decaps(device, param, count, dk.data(), ct.data(), ss.data()), "mlkem_decaps");
  return ss;
}
// one byte per instance: 1 = passes
inline std::vector<uint8_t> mlkem_check_ek(int device, int param, size_t count, const std::vector<uint8_t>& ek) {
  if (ek.size() != count * mlkem_sizes(param).ek) throw PsfError(PSF_ERR_PARAM, "mlkem_check_ek");
  std::vector<uint8_t> ok(count);
  check(psf_mlkem_check_ek(device, param, count, ek.data(), ok.data()), "mlkem_check_ek");
  return ok;
}
inline std::vector<uint8_t> mlkem_check_dk(int device, int param, size_t count, const std::vector<uint8_t>& dk) {
  if (dk.size() != count * mlkem_sizes(param).dk) throw PsfError(PSF_ERR_PARAM, "mlkem_check_dk");
  std::vector<uint8_t> ok(count);
  check(psf_mlkem_check_dk(device, param, count, dk.data(), ok.data()), "mlkem_check_dk");
  return ok;
}

// ---- FIPS 204 stages and ML-DSA, batched (psf_*_fips204*, psf_mldsa_*; sizes, the workspace and the rules in psf_mi355x.h).  `param` is PSF_MLDSA_44 / _65 / _87
inline void sample_ntt_fips204_dev(int device, size_t count, uint32_t k, uint32_t l, const uint8_t* d_seed, size_t seed_stride, uint64_t* d_out, int* d_fail = nullptr,
                                   void* stream = nullptr) {
  check(psf_sample_ntt_fips204_dev(device, count, k, l, d_seed, seed_stride, d_out, d_fail, stream), "sample_ntt_fips204_dev");
}
inline void sample_bounded_fips204_dev(int device, size_t count, uint32_t eta, const uint8_t* d_seed, size_t seed_stride, uint32_t first_nonce, uint32_t per_seed,
                                       int64_t* d_out, int* d_fail = nullptr, void* stream = nullptr) {
  check(psf_sample_bounded_fips204_dev(device, count, eta, d_seed, seed_stride, first_nonce, per_seed, d_out, d_fail, stream), "sample_bounded_fips204_dev");
}
inline void sample_in_ball_fips204_dev(int device, size_t count, uint32_t tau, const uint8_t* d_ctilde, size_t ctilde_len, size_t ctilde_stride, int64_t* d_out,
                                       int* d_fail = nullptr, void* stream = nullptr) {
  check(psf_sample_in_ball_fips204_dev(device, count, tau, d_ctilde, ctilde_len, ctilde_stride, d_out, d_fail, stream), "sample_in_ball_fips204_dev");
}
inline void ntt_image_from_fips204_dev(int device, size_t count, const uint64_t* d_fhat, uint32_t* d_hat, void* stream = nullptr) {
  check(psf_ntt_image_from_fips204_dev(device, count, d_fhat, d_hat, stream), "ntt_image_from_fips204_dev");
}
// host forms: packed seeds in, 256 words per polynomial out
inline std::vector<uint64_t> sample_ntt_fips204(int device, size_t count, uint32_t k, uint32_t l, const std::vector<uint8_t>& seed) {
  if (seed.size() != count * (k ? 32 : 34)) throw PsfError(PSF_ERR_PARAM, "sample_ntt_fips204");
  std::vector<uint64_t> out(count * (k ? (size_t)k * l : 1) * 256);
  check(psf_sample_ntt_fips204(device, count, k, l, seed.data(), k ? 32 : 34, out.data()), "sample_ntt_fips204");
  return out;
}
inline std::vector<int64_t> sample_bounded_fips204(int device, size_t count, uint32_t eta, const std::vector<uint8_t>& seed, uint32_t first_nonce, uint32_t per_seed) {
  if (seed.size() != count * 64) throw PsfError(PSF_ERR_PARAM, "sample_bounded_fips204");
  std::vector<int64_t> out(count * per_seed * 256);
  check(psf_sample_bounded_fips204(device, count, eta, seed.data(), 64, first_nonce, per_seed, out.data()), "sample_bounded_fips204");
  return out;
}
inline std::vector<int64_t> sample_in_ball_fips204(int device, size_t count, uint32_t tau, const std::vector<uint8_t>& ctilde, size_t ctilde_len) {
  if (ctilde.size() != count * ctilde_len) throw PsfError(PSF_ERR_PARAM, "sample_in_ball_fips204");
  std::vector<int64_t> out(count * 256);
  check(psf_sample_in_ball_fips204(device, count, tau, ctilde.data(), ctilde_len, ctilde_len, out.data()), "sample_in_ball_fips204");
  return out;
}
inline std::vector<uint32_t> ntt_image_from_fips204(int device, size_t count, const std::vector<uint64_t>& fhat) {
  if (fhat.size() != count * 256) throw PsfError(PSF_ERR_PARAM, "ntt_image_from_fips204");
  std::vector<uint32_t> hat(count * 256);
  check(psf_ntt_image_from_fips204(device, count, fhat.data(), hat.data()), "ntt_image_from_fips204");
  return hat;
}
struct MlDsaSizes { size_t pk, sk, sig; };
inline MlDsaSizes mldsa_sizes(int param) {
  MlDsaSizes s{};
  check(psf_mldsa_sizes(param, &s.pk, &s.sk, &s.sig), "mldsa_sizes");
  return s;
}
inline size_t mldsa_workspace_bytes(int param, size_t count, int op) {
  size_t bytes = 0;
  check(psf_mldsa_workspace_bytes(param, count, op, &bytes), "mldsa_workspace_bytes");
  return bytes;
}
inline void mldsa_keygen_dev(int device, int param, size_t count, const uint8_t* d_xi, uint8_t* d_pk, uint8_t* d_sk, void* d_ws, size_t ws_bytes, int* d_fail = nullptr,
                             void* stream = nullptr) {
  check(psf_mldsa_keygen_dev(device, param, count, d_xi, d_pk, d_sk, d_ws, ws_bytes, d_fail, stream), "mldsa_keygen_dev");
}
// pk_stride = 0: one key for all; msg_kind PSF_MLDSA_MSG_BYTES (M') or PSF_MLDSA_MSG_MU (msg_len = 64); d_why may be NULL
inline void mldsa_verify_dev(int device, int param, size_t count, const uint8_t* d_pk, size_t pk_stride, const uint8_t* d_msg, size_t msg_len, size_t msg_stride,
                             int msg_kind, const uint8_t* d_sig, uint8_t* d_ok, uint8_t* d_why, void* d_ws, size_t ws_bytes, int* d_fail = nullptr, void* stream = nullptr) {
  check(psf_mldsa_verify_dev(device, param, count, d_pk, pk_stride, d_msg, msg_len, msg_stride, msg_kind, d_sig, d_ok, d_why, d_ws, ws_bytes, d_fail, stream),
        "mldsa_verify_dev");
}
// host buffers, packed: xi 32 bytes per instance; returns (pk, sk)
inline std::pair<std::vector<uint8_t>, std::vector<uint8_t>> mldsa_keygen(int device, int param, size_t count, const std::vector<uint8_t>& xi) {
  const MlDsaSizes s = mldsa_sizes(param);
  if (xi.size() != count * 32) throw PsfError(PSF_ERR_PARAM, "mldsa_keygen");
  std::vector<uint8_t> pk(count * s.pk), sk(count * s.sk);
  check(psf_mldsa_keygen(device, param, count, xi.data(), pk.data(), sk.data()), "mldsa_keygen");
  return {pk, sk};
}
// pk: one key (for all) or count keys, packed; msg: count messages of msg_len bytes, packed; returns (ok, why), one byte per instance each
inline std::pair<std::vector<uint8_t>, std::vector<uint8_t>> mldsa_verify(int device, int param, size_t count, const std::vector<uint8_t>& pk, const std::vector<uint8_t>& msg,
                                                                          size_t msg_len, int msg_kind, const std::vector<uint8_t>& sig) {
  const MlDsaSizes s = mldsa_sizes(param);
  const bool one = pk.size() == s.pk && count != 1;
  if ((!one && pk.size() != count * s.pk) || msg.size() != count * msg_len || sig.size() != count * s.sig) throw PsfError(PSF_ERR_PARAM, "mldsa_verify");
  std::vector<uint8_t> ok(count), why(count);
  check(psf_mldsa_verify(device, param, count, pk.data(), one ? 0 : s.pk, msg.data(), msg_len, msg_len, msg_kind, sig.data(), ok.data(), why.data()), "mldsa_verify");
  return {ok, why};
}
// signing: begin, then rounds with `active` = the value last read from *d_live until it is 0, then end (psf_mi355x.h); sk_stride = 0: one key for all
inline size_t mldsa_sign_workspace_bytes(int param, size_t count, size_t sk_stride) {
  size_t bytes = 0;
  check(psf_mldsa_sign_workspace_bytes(param, count, sk_stride, &bytes), "mldsa_sign_workspace_bytes");
  return bytes;
}
inline void mldsa_sign_begin_dev(int device, int param, size_t count, const uint8_t* d_sk, size_t sk_stride, const uint8_t* d_msg, size_t msg_len, size_t msg_stride,
                                 int msg_kind, const uint8_t* d_rnd, void* d_ws, size_t ws_bytes, uint32_t* d_live, int* d_fail = nullptr, void* stream = nullptr) {
  check(psf_mldsa_sign_begin_dev(device, param, count, d_sk, sk_stride, d_msg, msg_len, msg_stride, msg_kind, d_rnd, d_ws, ws_bytes, d_live, d_fail, stream),
        "mldsa_sign_begin_dev");
}
inline void mldsa_sign_round_dev(int device, int param, size_t count, size_t sk_stride, size_t active, uint8_t* d_sig, uint32_t* d_rounds, void* d_ws, size_t ws_bytes,
                                 uint32_t* d_live, int* d_fail = nullptr, void* stream = nullptr) {
  check(psf_mldsa_sign_round_dev(device, param, count, sk_stride, active, d_sig, d_rounds, d_ws, ws_bytes, d_live, d_fail, stream), "mldsa_sign_round_dev");
}
inline void mldsa_sign_end_dev(int device, int param, size_t count, size_t sk_stride, void* d_ws, size_t ws_bytes, void* stream = nullptr) {
  check(psf_mldsa_sign_end_dev(device, param, count, sk_stride, d_ws, ws_bytes, stream), "mldsa_sign_end_dev");
}
// sk: one key (for all) or count keys, packed; msg packed; rnd: empty (deterministic) or 32 bytes per instance; returns (sig, rounds); throws
// PSF_ERR_SAMPLER when instances are unsigned after max_rounds rounds
inline std::pair<std::vector<uint8_t>, std::vector<uint32_t>> mldsa_sign(int device, int param, size_t count, const std::vector<uint8_t>& sk, const std::vector<uint8_t>& msg,
                                                                         size_t msg_len, int msg_kind, const std::vector<uint8_t>& rnd, uint32_t max_rounds = 1024) {
  const MlDsaSizes s = mldsa_sizes(param);
  const bool one = sk.size() == s.sk && count != 1;
  if ((!one && sk.size() != count * s.sk) || msg.size() != count * msg_len || (!rnd.empty() && rnd.size() != count * 32)) throw PsfError(PSF_ERR_PARAM, "mldsa_sign");
  std::vector<uint8_t> sig(count * s.sig);
  std::vector<uint32_t> rounds(count);
  check(psf_mldsa_sign(device, param, count, sk.data(), one ? 0 : s.sk, msg.data(), msg_len, msg_len, msg_kind, rnd.empty() ? nullptr : rnd.data(), sig.data(), max_rounds,
                       rounds.data()),
        "mldsa_sign");
  return {sig, rounds};
}

// ---- SLH-DSA, batched (psf_slhdsa_*; sizes, the workspace and the rules in psf_mi355x.h).  `param` is PSF_SLHDSA_SHAKE_128S ... _256F
struct SlhDsaSizes { size_t pk, sk, sig; };
inline SlhDsaSizes slhdsa_sizes(int param) {
  SlhDsaSizes s{};
  check(psf_slhdsa_sizes(param, &s.pk, &s.sk, &s.sig), "slhdsa_sizes");
  return s;
}
inline size_t slhdsa_workspace_bytes(int param, size_t count, int op) {
  size_t bytes = 0;
  check(psf_slhdsa_workspace_bytes(param, count, op, &bytes), "slhdsa_workspace_bytes");
  return bytes;
}
inline void slhdsa_keygen_dev(int device, int param, size_t count, const uint8_t* d_sk_seed, const uint8_t* d_sk_prf, const uint8_t* d_pk_seed, uint8_t* d_pk, uint8_t* d_sk,
                              void* d_ws, size_t ws_bytes, void* stream = nullptr) {
  check(psf_slhdsa_keygen_dev(device, param, count, d_sk_seed, d_sk_prf, d_pk_seed, d_pk, d_sk, d_ws, ws_bytes, stream), "slhdsa_keygen_dev");
}
// pk_stride = 0: one key for all
inline void slhdsa_verify_dev(int device, int param, size_t count, const uint8_t* d_pk, size_t pk_stride, const uint8_t* d_msg, size_t msg_len, size_t msg_stride,
                              const uint8_t* d_sig, uint8_t* d_ok, void* d_ws, size_t ws_bytes, void* stream = nullptr) {
  check(psf_slhdsa_verify_dev(device, param, count, d_pk, pk_stride, d_msg, msg_len, msg_stride, d_sig, d_ok, d_ws, ws_bytes, stream), "slhdsa_verify_dev");
}
// host buffers, packed: n = pk / 2 bytes of each seed per instance; returns (pk, sk)
inline std::pair<std::vector<uint8_t>, std::vector<uint8_t>> slhdsa_keygen(int device, int param, size_t count, const std::vector<uint8_t>& sk_seed,
                                                                           const std::vector<uint8_t>& sk_prf, const std::vector<uint8_t>& pk_seed) {
  const SlhDsaSizes s = slhdsa_sizes(param);
  const size_t n = s.pk / 2;
  if (sk_seed.size() != count * n || sk_prf.size() != count * n || pk_seed.size() != count * n) throw PsfError(PSF_ERR_PARAM, "slhdsa_keygen");
  std::vector<uint8_t> pk(count * s.pk), sk(count * s.sk);
  check(psf_slhdsa_keygen(device, param, count, sk_seed.data(), sk_prf.data(), pk_seed.data(), pk.data(), sk.data()), "slhdsa_keygen");
  return {pk, sk};
}
// pk: one key (for all) or count keys, packed; msg: count messages of msg_len bytes, packed; returns ok, one byte per instance
inline std::vector<uint8_t> slhdsa_verify(int device, int param, size_t count, const std::vector<uint8_t>& pk, const std::vector<uint8_t>& msg, size_t msg_len,
                                          const std::vector<uint8_t>& sig) {
  const SlhDsaSizes s = slhdsa_sizes(param);
  const bool one = pk.size() == s.pk && count != 1;
  if ((!one && pk.size() != count * s.pk) || msg.size() != count * msg_len || sig.size() != count * s.sig) throw PsfError(PSF_ERR_PARAM, "slhdsa_verify");
  std::vector<uint8_t> ok(count);
  check(psf_slhdsa_verify(device, param, count, pk.data(), one ? 0 : s.pk, msg.data(), msg_len, msg_len, sig.data(), ok.data()), "slhdsa_verify");
  return ok;
}
// signing (Algorithm 19); sk_stride = 0: one key for all; d_addrnd NULL: the deterministic variant
inline size_t slhdsa_sign_workspace_bytes(int param, size_t count) {
  size_t bytes = 0;
  check(psf_slhdsa_sign_workspace_bytes(param, count, &bytes), "slhdsa_sign_workspace_bytes");
  return bytes;
}
inline void slhdsa_sign_dev(int device, int param, size_t count, const uint8_t* d_sk, size_t sk_stride, const uint8_t* d_msg, size_t msg_len, size_t msg_stride,
                            const uint8_t* d_addrnd, uint8_t* d_sig, void* d_ws, size_t ws_bytes, void* stream = nullptr) {
  check(psf_slhdsa_sign_dev(device, param, count, d_sk, sk_stride, d_msg, msg_len, msg_stride, d_addrnd, d_sig, d_ws, ws_bytes, stream), "slhdsa_sign_dev");
}
// sk: one key (for all) or count keys, packed; msg: count messages of msg_len bytes, packed; addrnd: empty (deterministic) or count * n bytes; returns
// the signatures, packed
inline std::vector<uint8_t> slhdsa_sign(int device, int param, size_t count, const std::vector<uint8_t>& sk, const std::vector<uint8_t>& msg, size_t msg_len,
                                        const std::vector<uint8_t>& addrnd = {}) {
  const SlhDsaSizes s = slhdsa_sizes(param);
  const bool one = sk.size() == s.sk && count != 1;
  if ((!one && sk.size() != count * s.sk) || msg.size() != count * msg_len || (!addrnd.empty() && addrnd.size() != count * (s.pk / 2)))
    throw PsfError(PSF_ERR_PARAM, "slhdsa_sign");
  std::vector<uint8_t> sig(count * s.sig);
  check(psf_slhdsa_sign(device, param, count, sk.data(), one ? 0 : s.sk, msg.data(), msg_len, msg_len, addrnd.empty() ? nullptr : addrnd.data(), sig.data()),
        "slhdsa_sign");
  return sig;
}

// ---- SLH-DSA for the SHA-2 parameter sets, batched (psf_slhdsa_sha2_*: KeyGen, Verify and signing; rules in psf_mi355x.h).  `param` is PSF_SLHDSA_SHA2_128S ... _256F
inline SlhDsaSizes slhdsa_sha2_sizes(int param) {
  SlhDsaSizes s{};
  check(psf_slhdsa_sha2_sizes(param, &s.pk, &s.sk, &s.sig), "slhdsa_sha2_sizes");
  return s;
}
inline size_t slhdsa_sha2_workspace_bytes(int param, size_t count, int op) {
  size_t bytes = 0;
  check(psf_slhdsa_sha2_workspace_bytes(param, count, op, &bytes), "slhdsa_sha2_workspace_bytes");
  return bytes;
}
inline void slhdsa_sha2_keygen_dev(int device, int param, size_t count, const uint8_t* d_sk_seed, const uint8_t* d_sk_prf, const uint8_t* d_pk_seed, uint8_t* d_pk, uint8_t* d_sk,
                              void* d_ws, size_t ws_bytes, void* stream = nullptr) {
  check(psf_slhdsa_sha2_keygen_dev(device, param, count, d_sk_seed, d_sk_prf, d_pk_seed, d_pk, d_sk, d_ws, ws_bytes, stream), "slhdsa_sha2_keygen_dev");
}
// pk_stride = 0: one key for all
inline void slhdsa_sha2_verify_dev(int device, int param, size_t count, const uint8_t* d_pk, size_t pk_stride, const uint8_t* d_msg, size_t msg_len, size_t msg_stride,
                              const uint8_t* d_sig, uint8_t* d_ok, void* d_ws, size_t ws_bytes, void* stream = nullptr) {
  check(psf_slhdsa_sha2_verify_dev(device, param, count, d_pk, pk_stride, d_msg, msg_len, msg_stride, d_sig, d_ok, d_ws, ws_bytes, stream), "slhdsa_sha2_verify_dev");
}
// host buffers, packed: n = pk / 2 bytes of each seed per instance; returns (pk, sk)
inline std::pair<std::vector<uint8_t>, std::vector<uint8_t>> slhdsa_sha2_keygen(int device, int param, size_t count, const std::vector<uint8_t>& sk_seed,
                                                                           const std::vector<uint8_t>& sk_prf, const std::vector<uint8_t>& pk_seed) {
  const SlhDsaSizes s = slhdsa_sha2_sizes(param);
  const size_t n = s.pk / 2;
  if (sk_seed.size() != count * n || sk_prf.size() != count * n || pk_seed.size() != count * n) throw PsfError(PSF_ERR_PARAM, "slhdsa_sha2_keygen");
  std::vector<uint8_t> pk(count * s.pk), sk(count * s.sk);
  check(psf_slhdsa_sha2_keygen(device, param, count, sk_seed.data(), sk_prf.data(), pk_seed.data(), pk.data(), sk.data()), "slhdsa_sha2_keygen");
  return {pk, sk};
}
// pk: one key (for all) or count keys, packed; msg: count messages of msg_len bytes, packed; returns ok, one byte per instance
inline std::vector<uint8_t> slhdsa_sha2_verify(int device, int param, size_t count, const std::vector<uint8_t>& pk, const std::vector<uint8_t>& msg, size_t msg_len,
                                          const std::vector<uint8_t>& sig) {
  const SlhDsaSizes s = slhdsa_sha2_sizes(param);
  const bool one = pk.size() == s.pk && count != 1;
  if ((!one && pk.size() != count * s.pk) || msg.size() != count * msg_len || sig.size() != count * s.sig) throw PsfError(PSF_ERR_PARAM, "slhdsa_sha2_verify");
  std::vector<uint8_t> ok(count);
  check(psf_slhdsa_sha2_verify(device, param, count, pk.data(), one ? 0 : s.pk, msg.data(), msg_len, msg_len, sig.data(), ok.data()), "slhdsa_sha2_verify");
  return ok;
}
// signing (Algorithm 19); sk_stride = 0: one key for all; d_addrnd NULL: the deterministic variant
inline size_t slhdsa_sha2_sign_workspace_bytes(int param, size_t count) {
  size_t bytes = 0;
  check(psf_slhdsa_sha2_sign_workspace_bytes(param, count, &bytes), "slhdsa_sha2_sign_workspace_bytes");
  return bytes;
}
inline void slhdsa_sha2_sign_dev(int device, int param, size_t count, const uint8_t* d_sk, size_t sk_stride, const uint8_t* d_msg, size_t msg_len, size_t msg_stride,
                                 const uint8_t* d_addrnd, uint8_t* d_sig, void* d_ws, size_t ws_bytes, void* stream = nullptr) {
  check(psf_slhdsa_sha2_sign_dev(device, param, count, d_sk, sk_stride, d_msg, msg_len, msg_stride, d_addrnd, d_sig, d_ws, ws_bytes, stream), "slhdsa_sha2_sign_dev");
}
// sk: one key (for all) or count keys, packed; msg: count messages of msg_len bytes, packed; addrnd: empty (deterministic) or count * n bytes; returns
// the signatures, packed
inline std::vector<uint8_t> slhdsa_sha2_sign(int device, int param, size_t count, const std::vector<uint8_t>& sk, const std::vector<uint8_t>& msg, size_t msg_len,
                                             const std::vector<uint8_t>& addrnd = {}) {
  const SlhDsaSizes s = slhdsa_sha2_sizes(param);
  const bool one = sk.size() == s.sk && count != 1;
  if ((!one && sk.size() != count * s.sk) || msg.size() != count * msg_len || (!addrnd.empty() && addrnd.size() != count * (s.pk / 2)))
    throw PsfError(PSF_ERR_PARAM, "slhdsa_sha2_sign");
  std::vector<uint8_t> sig(count * s.sig);
  check(psf_slhdsa_sha2_sign(device, param, count, sk.data(), one ? 0 : s.sk, msg.data(), msg_len, msg_len, addrnd.empty() ? nullptr : addrnd.data(), sig.data()),
        "slhdsa_sha2_sign");
  return sig;
}

// ---- PSFPerturbation (mp_perturbation.rs:57-62, :193-403) -------------------------------------------------------------
class PSFPerturbation {
 public:
  struct Trapdoor { std::vector<int8_t> R; std::vector<double> sqrt_sigma_2; MatZ Sk; std::vector<double> Sk_gso; };   // :195

  PSFPerturbation(const psf_gadget_params& gp, double r, double s, int device = 0) : gp_(gp) {
    psfp_params p{gp, r, s, device, 0};
    check(psfp_create(&p, &h_), "PSFPerturbation");
  }
  ~PSFPerturbation() { psfp_destroy(h_); }
  PSFPerturbation(const PSFPerturbation&) = delete;
  PSFPerturbation& operator=(const PSFPerturbation&) = delete;

  size_t n() const { return gp_.n; }
  size_t m() const { return psfp_m(h_); }

  std::pair<MatZq, Trapdoor> trap_gen(uint64_t seed) {                                          // :221-244
    check(psfp_trap_gen(h_, seed), "trap_gen");
    const size_t mm = m(), w = gp_.n * gp_.k;
    MatZq A(gp_.n * mm);
    Trapdoor td;
    td.R.resize(gp_.m_bar * w); td.sqrt_sigma_2.resize(mm * (mm + 1) / 2); td.Sk.resize(gp_.k * gp_.k); td.Sk_gso.resize(gp_.k * gp_.k);
    check(psfp_export_key(h_, A.data(), td.R.data(), td.sqrt_sigma_2.data()), "export_key");
    check(psfp_export_gadget_basis(h_, td.Sk.data(), td.Sk_gso.data()), "export_gadget_basis");
    return {std::move(A), std::move(td)};
  }
  void load_key(const MatZq& A, const Trapdoor& td) { check(psfp_load_key(h_, A.data(), td.R.data(), td.sqrt_sigma_2.data()), "load_key"); }
  void load_public_key(const MatZq& A) { check(psfp_load_key(h_, A.data(), nullptr, nullptr), "load_key"); }      // a verifier's handle: f_a / check_domain only
  // (A, R) without a factor and without computing one: what compute_sqrt_sigma_2 (a pure function of mat_r and mat_sigma, :111) starts from; A may be null
  void load_trapdoor(const std::vector<int8_t>& R, const MatZq* A = nullptr) { check(psfp_load_trapdoor(h_, A ? A->data() : nullptr, R.data()), "load_trapdoor"); }
  // compute_sqrt_sigma_2 (:111-139): Sigma = s_cov^2 I, or any symmetric covariance as its packed lower triangle (row i: i + 1 entries)
  void compute_sqrt_sigma_2(double s_cov) { check(psfp_compute_sqrt_sigma_2(h_, s_cov), "compute_sqrt_sigma_2"); }
  void compute_sqrt_sigma_2(const std::vector<double>& sigma_lower_packed) { check(psfp_compute_sqrt_sigma_2_dense(h_, sigma_lower_packed.data()), "compute_sqrt_sigma_2"); }
  MatZ samp_d(uint64_t seed, size_t B = 1, uint64_t first_index = 0) {                           // :264-267
    MatZ e(B * m());
    check(psfp_samp_d(h_, seed, first_index, B, e.data()), "samp_d");
    return e;
  }
  MatZ samp_p(const MatZq& u, uint64_t seed, uint64_t first_index = 0) {                         // :304-336
    const size_t B = u.size() / n();
    MatZ e(B * m());
    check(psfp_samp_p(h_, seed, first_index, B, u.data(), e.data()), "samp_p");
    return e;
  }
  // the same, asynchronous: e (B * m entries, caller-owned) is complete after wait(); at most two calls in flight per handle
  void samp_p_async(const MatZq& u, MatZ& e, uint64_t seed, uint64_t first_index = 0) {
    const size_t B = u.size() / n();
    e.resize(B * m());
    check(psfp_samp_p_async(h_, seed, first_index, B, u.data(), e.data()), "samp_p_async");
  }
  void wait() { check(psfp_wait(h_), "wait"); }
  // count = seeds.size() independent samp_p_dev calls in one submission on device buffers (d_u: count * B * n targets, d_e: count * B * m entries), ordered on `stream`
  // (a hipStream_t, nullptr = default); the bytes of the loop of single calls (include/psf_mi355x.h)
  void samp_p_dev_many(const uint64_t* d_u, int64_t* d_e, size_t B, const std::vector<uint64_t>& seeds, const std::vector<uint64_t>& first_indices, void* stream = nullptr) {
    if (seeds.size() != first_indices.size()) throw PsfError(PSF_ERR_PARAM, "samp_p_dev_many");
    check(psfp_samp_p_dev_many(h_, seeds.size(), seeds.data(), first_indices.data(), B, d_u, d_e, stream), "samp_p_dev_many");
  }
  MatZq f_a(const MatZ& sigma) {                                                                  // :366-369
    if (sigma.empty() || sigma.size() % m() != 0) throw PsfError(PSF_ERR_DOMAIN, "f_a");
    const size_t B = sigma.size() / m();
    MatZq u(B * n());
    check(psfp_f_a(h_, B, sigma.data(), u.data()), "f_a");
    return u;
  }
  bool check_domain(const MatZ& sigma) {                                                          // :396-402 (one vector)
    uint8_t ok = 0;
    check(psfp_check_domain(h_, 1, sigma.data(), sigma.size(), &ok), "check_domain");
    return ok != 0;
  }
  psfp_handle* raw() { return h_; }

 private:
  psf_gadget_params gp_;
  psfp_handle* h_ = nullptr;
};

// ---- PSFGPV (gpv.rs:53-57, :59-225) ------------------------------------------------------------------------------------------
class PSFGPV {
 public:
  struct Trapdoor { std::vector<int32_t> basis_t; std::vector<double> gso_t; };   // (short_base, short_base_gso) transposed, gpv.rs:61

  PSFGPV(const psf_gadget_params& gp, double s, int device = 0) : gp_(gp) {
    psfgpv_params p{gp, s, device, 0};
    check(psfgpv_create(&p, &h_), "PSFGPV");
  }
  ~PSFGPV() { psfgpv_destroy(h_); }
  PSFGPV(const PSFGPV&) = delete;
  PSFGPV& operator=(const PSFGPV&) = delete;
  size_t n() const { return gp_.n; }
  size_t m() const { return psfgpv_m(h_); }

  std::pair<MatZq, Trapdoor> trap_gen(uint64_t seed) {                                            // :83-94
    check(psfgpv_trap_gen(h_, seed), "trap_gen");
    const size_t mm = m();
    MatZq A(gp_.n * mm);
    Trapdoor td;
    td.basis_t.resize(mm * mm); td.gso_t.resize(mm * mm);
    check(psfgpv_export_key(h_, A.data(), nullptr, td.basis_t.data(), td.gso_t.data()), "export_key");
    return {std::move(A), std::move(td)};
  }
  void load_key(const MatZq& A, const Trapdoor& td) { check(psfgpv_load_key(h_, A.data(), td.basis_t.data(), td.gso_t.data()), "load_key"); }
  MatZ samp_d(uint64_t seed, size_t B = 1, uint64_t first_index = 0) {                            // :113-116
    MatZ e(B * m());
    check(psfgpv_samp_d(h_, seed, first_index, B, e.data()), "samp_d");
    return e;
  }
  MatZ samp_p(const MatZq& u, uint64_t seed, uint64_t first_index = 0) {                          // :152-161
    const size_t B = u.size() / n();
    MatZ e(B * m());
    check(psfgpv_samp_p(h_, seed, first_index, B, u.data(), e.data()), "samp_p");
    return e;
  }
  // the same, asynchronous: e (B * m entries, caller-owned) is complete after wait(); at most two calls in flight per handle
  void samp_p_async(const MatZq& u, MatZ& e, uint64_t seed, uint64_t first_index = 0) {
    const size_t B = u.size() / n();
    e.resize(B * m());
    check(psfgpv_samp_p_async(h_, seed, first_index, B, u.data(), e.data()), "samp_p_async");
  }
  void wait() { check(psfgpv_wait(h_), "wait"); }
  // count = seeds.size() independent samp_p_dev calls in one submission on device buffers (d_u: count * B * n targets, d_e: count * B * m entries), ordered on `stream`
  // (a hipStream_t, nullptr = default); the bytes of the loop of single calls (include/psf_mi355x.h)
  void samp_p_dev_many(const uint64_t* d_u, int64_t* d_e, size_t B, const std::vector<uint64_t>& seeds, const std::vector<uint64_t>& first_indices, void* stream = nullptr) {
    if (seeds.size() != first_indices.size()) throw PsfError(PSF_ERR_PARAM, "samp_p_dev_many");
    check(psfgpv_samp_p_dev_many(h_, seeds.size(), seeds.data(), first_indices.data(), B, d_u, d_e, stream), "samp_p_dev_many");
  }
  MatZq f_a(const MatZ& sigma) {                                                                   // :190-193
    if (sigma.empty() || sigma.size() % m() != 0) throw PsfError(PSF_ERR_DOMAIN, "f_a");
    const size_t B = sigma.size() / m();
    MatZq u(B * n());
    check(psfgpv_f_a(h_, B, sigma.data(), u.data()), "f_a");
    return u;
  }
  bool check_domain(const MatZ& sigma) {                                                           // :219-224
    uint8_t ok = 0;
    check(psfgpv_check_domain(h_, 1, sigma.data(), sigma.size(), &ok), "check_domain");
    return ok != 0;
  }

 private:
  psf_gadget_params gp_;
  psfgpv_handle* h_ = nullptr;
};

// ---- PSFGPVRing (gpv_ring.rs:62-67, :69-284); polynomials are n coefficients, constant term first ----------------------------
class PSFGPVRing {
 public:
  struct Trapdoor { MatZ r, e; };   // two 1 x k MatPolyOverZ, gpv_ring.rs:72

  PSFGPVRing(const psf_gadget_params& ring_gp, double s, double s_td, int device = 0) : gp_(ring_gp) {
    psfring_params p{ring_gp, s, s_td, device, 0};
    check(psfring_create(&p, &h_), "PSFGPVRing");
  }
  ~PSFGPVRing() { psfring_destroy(h_); }
  PSFGPVRing(const PSFGPVRing&) = delete;
  PSFGPVRing& operator=(const PSFGPVRing&) = delete;
  size_t n() const { return gp_.n; }
  size_t polys() const { return gp_.k + 2; }

  std::pair<MatZq, Trapdoor> trap_gen(uint64_t seed) {                                             // :91-98
    check(psfring_trap_gen(h_, seed), "trap_gen");
    MatZq a(polys() * n());
    Trapdoor td;
    td.r.resize(gp_.k * n()); td.e.resize(gp_.k * n());
    check(psfring_export_key(h_, a.data(), td.r.data(), td.e.data(), nullptr, nullptr), "export_key");
    return {std::move(a), std::move(td)};
  }
  void load_key(const MatZq& a, const Trapdoor& td) { check(psfring_load_key(h_, a.data(), td.r.data(), td.e.data()), "load_key"); }
  MatZ samp_d(uint64_t seed, size_t B = 1, uint64_t first_index = 0) {                             // :118-122
    MatZ sg(B * polys() * n());
    check(psfring_samp_d(h_, seed, first_index, B, sg.data()), "samp_d");
    return sg;
  }
  MatZ samp_p(const MatZq& u, uint64_t seed, uint64_t first_index = 0) {                           // :160-212
    const size_t B = u.size() / n();
    MatZ sg(B * polys() * n());
    check(psfring_samp_p(h_, seed, first_index, B, u.data(), sg.data()), "samp_p");
    return sg;
  }
  void samp_p_async(const MatZq& u, MatZ& sg, uint64_t seed, uint64_t first_index = 0) {           // sg is complete after wait()
    const size_t B = u.size() / n();
    sg.resize(B * polys() * n());
    check(psfring_samp_p_async(h_, seed, first_index, B, u.data(), sg.data()), "samp_p_async");
  }
  void wait() { check(psfring_wait(h_), "wait"); }
  // count = seeds.size() independent samp_p_dev calls in one submission on device buffers (d_u: count * B * n targets, d_sg: count * B * (k + 2) * n entries), ordered on `stream`
  // (a hipStream_t, nullptr = default); the bytes of the loop of single calls (include/psf_mi355x.h)
  void samp_p_dev_many(const uint64_t* d_u, int64_t* d_sg, size_t B, const std::vector<uint64_t>& seeds, const std::vector<uint64_t>& first_indices, void* stream = nullptr) {
    if (seeds.size() != first_indices.size()) throw PsfError(PSF_ERR_PARAM, "samp_p_dev_many");
    check(psfring_samp_p_dev_many(h_, seeds.size(), seeds.data(), first_indices.data(), B, d_u, d_sg, stream), "samp_p_dev_many");
  }
  MatZq f_a(const MatZ& sigma) {                                                                    // :243-247
    const size_t d = polys() * n();
    if (sigma.empty() || sigma.size() % d != 0) throw PsfError(PSF_ERR_DOMAIN, "f_a");
    MatZq u(sigma.size() / d * n());
    check(psfring_f_a(h_, sigma.size() / d, sigma.data(), u.data()), "f_a");
    return u;
  }
  bool check_domain(const MatZ& sigma) {                                                            // :274-283
    uint8_t ok = 0;
    check(psfring_check_domain(h_, 1, sigma.data(), sigma.size(), &ok), "check_domain");
    return ok != 0;
  }

 private:
  psf_gadget_params gp_;
  psfring_handle* h_ = nullptr;
};

}  // namespace psf_mi355x
