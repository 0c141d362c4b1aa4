/*
 * psf_mi355x.h -- C ABI of the MI355X-native preimage-sampling library (libpsf_mi355x.so).
 *
 * Drop-in boundary for ONE hot path of qfall/tools: the `PSF` trait (src/primitive/psf.rs:39-81)
 * as implemented by PSFPerturbation (src/primitive/psf/mp_perturbation.rs), PSFGPV (gpv.rs) and
 * PSFGPVRing (gpv_ring.rs), plus the gadget-lattice helpers under them
 * (src/sample/g_trapdoor/{gadget_classical,gadget_ring,short_basis_classical,short_basis_ring}.rs).
 * The reference has no FFI of its own for this path (it is Rust over qfall-math/FLINT); these entry
 * points are what a Rust `extern "C"` block implementing `PSF` would bind -- see INTEGRATION.md.
 *
 * Conventions
 *   - every function returns a psf_status; 0 = success.  The reference panics where this ABI returns
 *     a non-zero status (mp_perturbation.rs:190,315,333,367); a shim turns status != 0 into panic!.
 *   - matrices are flat, row-major; batches are "one row per call of the reference":
 *       u : B x n   (Range  = MatZq n x 1 per call,   least non-negative residues)
 *       e : B x m   (Domain = MatZ  m x 1 per call)
 *   - one reference call == one row.  Batching (B > 1) is this library's extension: B independent
 *     samp_p calls sharing (A, trapdoor).  Row b of a batch uses the randomness of global preimage
 *     index `first_index + b`, so results do not depend on how a job is sharded over GPUs.
 *   - randomness: the reference's trait takes no seed (psf.rs:48-80); here every sampling entry point
 *     takes a 64-bit seed keying Philox4x32-10 streams (DESIGN.md "Randomness contract").
 *   - `*_dev` variants take device pointers (HIP) and a hipStream_t (as void*); the plain variants
 *     take host pointers and do the copies themselves.
 *   - a handle is not thread-safe: one handle per host thread / HIP stream, mirroring the reference's
 *     !Send + !Sync PSF values (gadget_parameters.rs:51, trapdoor_distribution.rs:22).
 */
#ifndef PSF_MI355X_H
#define PSF_MI355X_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int psf_status;
enum {
  PSF_OK = 0,
  PSF_ERR_PARAM = 1,           /* malformed arguments (dimension / NULL / range)                         */
  PSF_ERR_NOT_PD = 2,          /* Sigma_2 not positive definite: mp_perturbation.rs:109-110              */
  PSF_ERR_DOMAIN = 3,          /* f_a on sigma outside D_n: assert! at mp_perturbation.rs:367, gpv.rs:191 */
  PSF_ERR_MODULUS = 4,         /* base^k < q: gadget_classical.rs:170-172                                */
  PSF_ERR_NO_SOLUTION = 5,     /* A x = u has no solution: gpv.rs:153-155 unwrap                         */
  PSF_ERR_NO_KEY = 6,          /* samp_p / f_a before trap_gen / load_key                                */
  PSF_ERR_HIP = 7,             /* HIP runtime error (no device, out of memory, launch failure)           */
  PSF_ERR_UNSUPPORTED = 8,     /* parameter combination outside what the kernels cover                   */
  PSF_ERR_SAMPLER = 9          /* a draw did not accept within 65 536 attempts (Gaussian far below the smoothing parameter), or an
                                  intermediate left its range (nearest-plane centre beyond 2^62 or first-pass representative beyond 2^53,
                                  perturbation beyond 2^23);
                                  the reference would keep computing -- DESIGN.md section 8, "Limits" */
};

const char* psf_status_string(psf_status);
/* "gfx950" etc. of the device the library would run on; PSF_ERR_HIP if none */
psf_status psf_device_info(int device, char* name, size_t name_len, int* compute_units);

/* ------------------------------------------------------------------------------------------------
 * GadgetParameters (gadget_parameters.rs:44-52); distribution is PlusMinusOneZero
 * (trapdoor_distribution.rs:52-53, :82-86) for the classical variants, SampleZ (:58-59) for the ring.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  uint64_t n;      /* security parameter / ring degree            */
  uint64_t k;      /* gadget length, ceil(log_base q) by default  */
  uint64_t m_bar;  /* n*k + ceil(log2 n)^2 (classical), k+2 (ring) */
  uint64_t base;   /* gadget base (2 by default)                  */
  uint64_t q;      /* modulus, 1 < q < 2^62                       */
} psf_gadget_params;

/* GadgetParameters::init_default (gadget_parameters.rs:113-133) */
psf_status psf_gadget_params_default(uint64_t n, uint64_t q, psf_gadget_params* out);
/* GadgetParametersRing::init_default (gadget_parameters.rs:165-185); modulus polynomial X^n + 1
 * (common_moduli.rs:41-48) */
psf_status psf_gadget_params_ring_default(uint64_t n, uint64_t q, psf_gadget_params* out);

/* ------------------------------------------------------------------------------------------------
 * Deterministic gadget helpers (host entry points; the batched digit decomposition runs on device)
 * ---------------------------------------------------------------------------------------------- */
/* gen_gadget_vec (gadget_classical.rs:128-136): out[k] = base^i */
psf_status psf_gen_gadget_vec(uint64_t k, uint64_t base, int64_t* out);
/* gen_gadget_mat (gadget_classical.rs:91-107): out[n x n*k] = I_n (x) g^t */
psf_status psf_gen_gadget_mat(uint64_t n, uint64_t k, uint64_t base, int64_t* out);
/* find_solution_gadget_mat (gadget_classical.rs:219-229; entry rule :169-182):
 * value[rows x cols] in Z_q -> out[k*rows x cols], out[k*j+i, c] = i-th base-`base` digit of value[j,c].
 * Runs the HIP digit-decomposition kernel.  PSF_ERR_MODULUS if base^k < q. */
psf_status psf_find_solution_gadget_mat(int device, const uint64_t* value, size_t rows, size_t cols,
                                        uint64_t q, uint64_t k, uint64_t base, int64_t* out);
/* short_basis_gadget (gadget_classical.rs:248-287): out[nk x nk] = I_n (x) S_k */
psf_status psf_short_basis_gadget(const psf_gadget_params* gp, int64_t* out);
/* gen_short_basis_for_trapdoor (short_basis_classical.rs:54-63), tag = identity when NULL:
 * out[m x m] = [I R; 0 I] * [0 I; S' W] */
psf_status psf_gen_short_basis_for_trapdoor(const psf_gadget_params* gp, const uint64_t* tag /*n x n*/,
                                            const uint64_t* A /*n x m*/, const int8_t* R /*m_bar x nk*/,
                                            int64_t* out);
/* gen_trapdoor (gadget_classical.rs:56-68) for a caller-supplied A_bar (n x m_bar) and tag H (n x n, NULL = identity, :61-66):
 * R <- PlusMinusOneZero (trapdoor_distribution.rs:82-86) from `seed`, A = [A_bar | H G - A_bar R] computed on the device.
 * PSF_ERR_MODULUS if base^k < q. */
psf_status psf_gen_trapdoor(int device, const psf_gadget_params* gp, const uint64_t* a_bar, const uint64_t* tag, uint64_t seed,
                            uint64_t* A /*n x m*/, int8_t* R /*m_bar x nk*/);
/* the same with the caller's own R (m_bar x nk, row-major) -- the draw of whatever TrapdoorDistribution the caller uses: the reference samples R through
 * the trait object `params.distribution` (gadget_classical.rs:62-64, gadget_parameters.rs:51, trapdoor_distribution.rs:21-48).  |R_ij| <= 127
 * (the trapdoor is an int8 operand of the matrix cores on the device), PSF_ERR_UNSUPPORTED otherwise.  Install the pair with psfp_load_key(A, R, NULL). */
psf_status psf_gen_trapdoor_with_r(int device, const psf_gadget_params* gp, const uint64_t* a_bar, const uint64_t* tag, const int64_t* R,
                                   uint64_t* A /*n x m*/);
/* gen_trapdoor_ring_lwe (gadget_ring.rs:62-81): r, e <- SampleZ(s) from `seed`, a = [1 | a_bar | g^t - (a_bar r + e)] in R_q
 * (gp from psf_gadget_params_ring_default; q < 2^62).  a_bar: n coefficients; a: (k+2) x n; r, e: k x n */
psf_status psf_gen_trapdoor_ring_lwe(int device, const psf_gadget_params* gp, const uint64_t* a_bar, double s, uint64_t seed,
                                     uint64_t* a, int64_t* r, int64_t* e);
/* the same with the caller's own r, e (gadget_ring.rs:69-70 draw them through `params.distribution`); |coefficients| <= 2^30 */
psf_status psf_gen_trapdoor_ring_lwe_with(int device, const psf_gadget_params* gp, const uint64_t* a_bar, const int64_t* r, const int64_t* e, uint64_t* a);
/* gen_gadget_ring (gadget_ring.rs:103-109): the k constant polynomials base^j, out[j] = constant term */
psf_status psf_gen_gadget_ring(uint64_t k, uint64_t base, int64_t* out);
/* find_solution_gadget_ring (gadget_ring.rs:145-166): u (n coefficients of an element of R_q) -> out[k x n], polynomial i = i-th digit
 * of every coefficient (index i + j k of the classical solution, :160) */
psf_status psf_find_solution_gadget_ring(int device, const uint64_t* u, size_t n, uint64_t q, uint64_t k, uint64_t base, int64_t* out);
/* gen_short_basis_for_trapdoor_ring (short_basis_ring.rs:64-79): out[(row * n(k+2) + col) * n + coeff], (k+2) x n(k+2) polynomials */
psf_status psf_gen_short_basis_for_trapdoor_ring(const psf_gadget_params* gp, const uint64_t* a, const int64_t* r, const int64_t* e, int64_t* out);
/* Gram-Schmidt orthogonalisation of the ROWS of an integer matrix on the device -- the `MatQ::gso` step of PSFGPV::trap_gen (gpv.rs:88-91) and of
 * MatPolyOverZ::sample_d (gpv_ring.rs:205), as a free function: basis_t[rows x width] (row i = basis vector i), out[rows x width] = b~_i.
 * Blocked, re-orthogonalised, FP64 matrix cores (psf_gemm_kernels.hpp).  PSF_ERR_PARAM if the rows are linearly dependent. */
psf_status psf_gso_rows(int device, const int32_t* basis_t, size_t rows, size_t width, double* out);
/* contiguous shares of `total` rows over `world` workers; the first total % world workers get one row more */
psf_status psf_shard_range(size_t total, int world, int rank, size_t* first, size_t* count);
/* PolynomialRingZq product in R_q = Z_q[X]/(X^n + 1) (common_moduli.rs:41-48), the arithmetic under the MatPolynomialRingZq
 * products at gadget_ring.rs:78 and gpv_ring.rs:245-246: out[c] = a[c] * b[c] mod (X^n + 1, q) for `count` pairs of n
 * coefficients (constant term first); a as residues, b as signed integers (a MatPolyOverZ entry).  Runs on the device. */
psf_status psf_poly_mul_negacyclic(int device, uint64_t q, size_t n, size_t count, const uint64_t* a, const int64_t* b, uint64_t* out);
/* the same product with the method chosen explicitly: method 0 = schoolbook kernel, 1 = (incomplete) negacyclic NTT kernel,
 * available when q < 2^31 is a prime with 4 | q-1 and n is a power of two (q = 3329, n = 256: seven levels and degree-1
 * leaves, as in ML-KEM); PSF_ERR_UNSUPPORTED otherwise.  psf_poly_mul_negacyclic uses the NTT whenever it is available. */
psf_status psf_poly_mul_negacyclic_method(int device, uint64_t q, size_t n, size_t count, const uint64_t* a, const int64_t* b, uint64_t* out, int method);
/* The same product on DEVICE buffers in the caller's stream, nothing allocated per call (the tables of a (device, q, n) are built at first use and
 * kept): `count` products d_out[c] = d_a[c] * d_b[c] (PolynomialRingZq multiplication, gadget_ring.rs:78, gpv_ring.rs:245-246).
 *   io_bits = 64: the layout above (a uint64 of any value, b int64 of any value, out uint64 in [0, q)); every modulus below 2^62 (NTT when q is an
 *                 NTT-friendly prime below 2^31, the schoolbook kernel otherwise).
 *   io_bits = 16: a uint16 in [0, q), b int16 in (-q, q), out uint16 in [0, q) -- a quarter of the bytes; NTT-friendly primes q < 2^14
 *                 (3329, 7681, 12289: common_moduli.rs:41-48) with n = 128 ... 1024; PSF_ERR_UNSUPPORTED otherwise.
 * One 128 ... 1024-point transform per WAVEFRONT: every butterfly in registers, lane bits exchanged by DPP / permlane swaps, Montgomery
 * arithmetic (R = 2^16 on 24-bit multiplies for q < 2^14, R = 2^32 above), no division and no barrier (tools_amd/csrc/psf_ntt_core.hpp). */
psf_status psf_poly_mul_negacyclic_dev(int device, uint64_t q, size_t n, size_t count, const void* d_a, const void* d_b, void* d_out, int io_bits, void* stream);
/* A polynomial that takes part in many products (a key: a_bar of gadget_ring.rs:78, a of gpv_ring.rs:245) is transformed ONCE:
 * psf_ntt_forward_dev writes its image (count * n 32-bit words, opaque), psf_poly_mul_hat_dev multiplies images by polynomials: d_out[c] =
 * image[c * hat_stride ...] * d_b[c]; hat_stride in words, 0 = one image for every product.  Shapes with a wave kernel only (q an NTT-friendly
 * prime < 2^31, n = 128 ... 1024, leaf degree <= 4); PSF_ERR_UNSUPPORTED otherwise. */
psf_status psf_ntt_forward_dev(int device, uint64_t q, size_t n, size_t count, const void* d_a, int io_bits, uint32_t* d_hat, void* stream);
psf_status psf_poly_mul_hat_dev(int device, uint64_t q, size_t n, size_t count, const uint32_t* d_hat, size_t hat_stride, const void* d_b, void* d_out, int io_bits,
                                void* stream);
/* MatPolynomialRingZq * MatPolynomialRingZq (gpv_ring.rs:245, gadget_ring.rs:78 and :190-202, short_basis_ring.rs:183-198):
 * C[c] = op(A[c]) . B[c] over R_q = Z_q[X]/(X^n + 1), for c < count, on DEVICE buffers in the caller's stream, nothing allocated per call.
 * Matrices of polynomials are row-major; each polynomial is n coefficients, constant term first.
 *   A[c]: at d_a + c * a_stride polynomials; a_stride = 0 means one A for every batch.
 *         trans_a = 0: A is rows x inner and op(A) = A;  trans_a = 1: A is stored inner x rows and op(A) = A^T.
 *   B[c]: inner x cols, contiguous after B[c-1].   C[c]: rows x cols, contiguous after C[c-1].
 *   io_bits = 64: a uint64 (any value), b int64 (any value), out uint64 in [0, q); every 2 <= q < 2^62 and n <= 8192.
 *   io_bits = 16: the 16-bit contract of psf_poly_mul_negacyclic_dev (a uint16 in [0, q), b int16 in (-q, q), out uint16); NTT primes q < 2^14 with
 *                 n = 128 ... 1024 (a wave kernel), PSF_ERR_UNSUPPORTED otherwise.
 * Exact for every inner <= 2^20 (PSF_ERR_UNSUPPORTED above).  When (q, n) has a wave kernel, one wave owns (batch, output column, tile of output
 * rows): B[c][k][j] is transformed once per tile, the leaf products are summed at one Montgomery scale, and each output polynomial takes one inverse
 * transform.  Every other q runs an exact schoolbook kernel.
 * PSF_ERR_PARAM: q <= 1 or q >= 2^62, n outside 1 ... 8192 (the codes of the pair product), rows, inner or cols = 0, trans_a not 0 / 1, io_bits not 16 / 64,
 * a NULL pointer when count > 0, a byte count that overflows size_t, or an output range that overlaps an input range.  count = 0 is PSF_OK.
 * Every check runs before the first HIP call; on PSF_ERR_PARAM / PSF_ERR_UNSUPPORTED nothing is launched and nothing is written.  A valid call
 * without a device is PSF_ERR_HIP (no CPU fallback). */
psf_status psf_matpoly_mul_negacyclic_dev(int device, uint64_t q, size_t n, size_t count, size_t rows, size_t inner, size_t cols, const void* d_a, size_t a_stride,
                                          int trans_a, const void* d_b, void* d_c, int io_bits, void* stream);
/* The same with A given by its images from psf_ntt_forward_dev (rows * inner images per batch, in A's storage order).  hat_stride is in 32-bit words;
 * 0 means one set of images for every batch (staged in LDS when its rows * inner * n words fit).  The shapes of psf_poly_mul_hat_dev only. */
psf_status psf_matpoly_mul_hat_dev(int device, uint64_t q, size_t n, size_t count, size_t rows, size_t inner, size_t cols, const uint32_t* d_hat, size_t hat_stride,
                                   int trans_a, const void* d_b, void* d_c, int io_bits, void* stream);
/* host buffers, one product C = A . B (rows x inner, inner x cols -> rows x cols); allocates per call, like psf_poly_mul_negacyclic */
psf_status psf_matpoly_mul_negacyclic(int device, uint64_t q, size_t n, size_t rows, size_t inner, size_t cols, const uint64_t* a, const int64_t* b, uint64_t* c);
/* The cyclic ring R_q = Z_q[X]/(X^n - 1) (new_cyclic, common_moduli.rs:72-79): one twin per X^n + 1 entry point above, with the same arguments,
 * layouts, word widths, limits, return codes and rules (every check before the first HIP call, nothing written on PSF_ERR_PARAM / PSF_ERR_UNSUPPORTED,
 * PSF_ERR_HIP without a device, no CPU fallback).  out[c] = sum_i a_i b_{(c - i) mod n}.  A (q, n) has a cyclic NTT exactly when it has a negacyclic
 * one: the same wave and LDS kernels run with a table of zetas for X^n - 1; every other q < 2^62 at 64-bit words runs an exact schoolbook kernel.
 * Images from psf_ntt_forward_cyclic_dev are opaque and valid only for the *_hat_cyclic_dev products (not for psf_poly_mul_hat_dev /
 * psf_matpoly_mul_hat_dev, and images from psf_ntt_forward_dev are not valid here). */
psf_status psf_poly_mul_cyclic(int device, uint64_t q, size_t n, size_t count, const uint64_t* a, const int64_t* b, uint64_t* out);
psf_status psf_poly_mul_cyclic_method(int device, uint64_t q, size_t n, size_t count, const uint64_t* a, const int64_t* b, uint64_t* out, int method);
psf_status psf_poly_mul_cyclic_dev(int device, uint64_t q, size_t n, size_t count, const void* d_a, const void* d_b, void* d_out, int io_bits, void* stream);
psf_status psf_ntt_forward_cyclic_dev(int device, uint64_t q, size_t n, size_t count, const void* d_a, int io_bits, uint32_t* d_hat, void* stream);
psf_status psf_poly_mul_hat_cyclic_dev(int device, uint64_t q, size_t n, size_t count, const uint32_t* d_hat, size_t hat_stride, const void* d_b, void* d_out,
                                       int io_bits, void* stream);
psf_status psf_matpoly_mul_cyclic_dev(int device, uint64_t q, size_t n, size_t count, size_t rows, size_t inner, size_t cols, const void* d_a, size_t a_stride,
                                      int trans_a, const void* d_b, void* d_c, int io_bits, void* stream);
psf_status psf_matpoly_mul_hat_cyclic_dev(int device, uint64_t q, size_t n, size_t count, size_t rows, size_t inner, size_t cols, const uint32_t* d_hat,
                                          size_t hat_stride, int trans_a, const void* d_b, void* d_c, int io_bits, void* stream);
psf_status psf_matpoly_mul_cyclic(int device, uint64_t q, size_t n, size_t rows, size_t inner, size_t cols, const uint64_t* a, const int64_t* b, uint64_t* c);
/* Fused multiply-add over R_q: C[c] = E[c] + sign * op(A[c]) B[c] for c < count -- t = A s + e, u = A^T r + e1, v = t^T r + e2, w = v - s^T u in one
 * launch each, and the checks a S (gadget_ring.rs:190-202) and A e - u with their subtraction.  One twin per matrix-product entry point above, with two
 * more arguments in front of the output: E[c] is rows x cols polynomials laid out like C[c], in B's word type and value contract (int64 of any value at
 * 64-bit words, int16 in (-q, q) at 16-bit words: signed noise and residues in [0, q) both fit); sign is +1 or -1, anything else PSF_ERR_PARAM.  C is
 * canonical, in [0, q).  The word of E is added in the kernel that finishes the output polynomial, by the thread that writes that word of C, so
 * d_e == d_c (exact in-place accumulation) is allowed; any other overlap of C with E is PSF_ERR_PARAM, like C overlapping A or B.  A NULL d_e with
 * count > 0 is PSF_ERR_PARAM.  Every other rule of psf_matpoly_mul_negacyclic_dev carries over: limits, codes, PSF_ERR_PARAM before
 * PSF_ERR_UNSUPPORTED, every check before the first HIP call, nothing written on error, no allocation, no synchronisation, count = 0 is PSF_OK.
 * The host-buffer forms take one batch and allow c == e. */
psf_status psf_matpoly_mul_add_negacyclic_dev(int device, uint64_t q, size_t n, size_t count, size_t rows, size_t inner, size_t cols, const void* d_a, size_t a_stride,
                                              int trans_a, const void* d_b, const void* d_e, int sign, void* d_c, int io_bits, void* stream);
psf_status psf_matpoly_mul_add_hat_dev(int device, uint64_t q, size_t n, size_t count, size_t rows, size_t inner, size_t cols, const uint32_t* d_hat, size_t hat_stride,
                                       int trans_a, const void* d_b, const void* d_e, int sign, void* d_c, int io_bits, void* stream);
psf_status psf_matpoly_mul_add_negacyclic(int device, uint64_t q, size_t n, size_t rows, size_t inner, size_t cols, const uint64_t* a, const int64_t* b, const int64_t* e,
                                          int sign, uint64_t* c);
psf_status psf_matpoly_mul_add_cyclic_dev(int device, uint64_t q, size_t n, size_t count, size_t rows, size_t inner, size_t cols, const void* d_a, size_t a_stride,
                                          int trans_a, const void* d_b, const void* d_e, int sign, void* d_c, int io_bits, void* stream);
psf_status psf_matpoly_mul_add_hat_cyclic_dev(int device, uint64_t q, size_t n, size_t count, size_t rows, size_t inner, size_t cols, const uint32_t* d_hat,
                                              size_t hat_stride, int trans_a, const void* d_b, const void* d_e, int sign, void* d_c, int io_bits, void* stream);
psf_status psf_matpoly_mul_add_cyclic(int device, uint64_t q, size_t n, size_t rows, size_t inner, size_t cols, const uint64_t* a, const int64_t* b, const int64_t* e,
                                      int sign, uint64_t* c);
/* R_q coefficient maps of the ML-KEM-style schemes, on a flat array of `len` coefficients (any number of polynomials, or of the entries of a
 * MatPolynomialRingZq, n coefficients each, constant term first).  Exact integer arithmetic, bit for bit against the big-integer definitions:
 *   compress   (LossyCompressionFIPS203::lossy_compress, lossy_compression_fips203.rs:89-112):   y = floor((x 2^d + floor(q/2)) / q) mod 2^d,
 *              x read as its residue mod q;
 *   decompress (lossy_decompress, :143-172):   x = floor((y q + 2^(d-1)) / 2^d) mod q for any signed y, written as the least non-negative
 *              residue (the reference stores the unreduced value, which can be q, or anything when y is outside [0, 2^d): the same element of R_q);
 *   encode     (encode_value_in_polynomialringzq, common_encodings.rs:49-91, after the base-`base` digits of the value): out = digit floor(q/base) mod q;
 *   decode     (decode_value_from_polynomialringzq, :125-151, before the digits are composed): digit = floor((base c + floor(q/(2 base))) / q) mod base,
 *              c read as its residue mod q.
 * Splitting a value into digits and composing digits into a value stay with the caller (tools_amd/encodings.py), as does reducing a PolyOverZ of
 * degree >= n.  Limits: 2 <= q < 2^62 (q < 2 PSF_ERR_PARAM, q >= 2^62 PSF_ERR_UNSUPPORTED); d < 1 PSF_ERR_PARAM (the reference panics), d > 63
 * PSF_ERR_UNSUPPORTED (a compressed value is an int64); base < 2 PSF_ERR_PARAM, base >= 2^63 PSF_ERR_UNSUPPORTED.  len = 0 is PSF_OK.  Every
 * argument is checked before the first HIP call.  The host-pointer forms run on the device (no CPU fallback; PSF_ERR_HIP without one). */
psf_status psf_lossy_compress(int device, uint64_t q, uint32_t d, size_t len, const uint64_t* x, int64_t* y);
psf_status psf_lossy_decompress(int device, uint64_t q, uint32_t d, size_t len, const int64_t* y, uint64_t* x);
psf_status psf_encode_digits(int device, uint64_t q, uint64_t base, size_t len, const uint64_t* digits, uint64_t* out);
psf_status psf_decode_digits(int device, uint64_t q, uint64_t base, size_t len, const uint64_t* coeffs, uint64_t* digits);
/* The same maps on DEVICE buffers, ordered on `stream`, nothing allocated per call.  io_bits = 64: the word types of the host forms;
 * io_bits = 16: uint16 words in and out (a compressed y is read mod 2^d, so signed or unsigned is the same), for q <= 2^16, d <= 16,
 * base <= 2^16 (PSF_ERR_UNSUPPORTED otherwise); any other io_bits PSF_ERR_PARAM.  Pointers need only the alignment of their word. */
psf_status psf_lossy_compress_dev(int device, uint64_t q, uint32_t d, size_t len, const void* d_x, void* d_y, int io_bits, void* stream);
psf_status psf_lossy_decompress_dev(int device, uint64_t q, uint32_t d, size_t len, const void* d_y, void* d_x, int io_bits, void* stream);
psf_status psf_encode_digits_dev(int device, uint64_t q, uint64_t base, size_t len, const void* d_digits, void* d_out, int io_bits, void* stream);
psf_status psf_decode_digits_dev(int device, uint64_t q, uint64_t base, size_t len, const void* d_coeffs, void* d_digits, int io_bits, void* stream);
/* FIPS 203 byte encodings of a flat array of `len` d-bit values, and their fusions with the compression maps above:
 *   byte_encode       (ByteEncode_d, Algorithm 5, for any len): nbytes = ceil(len d / 8) bytes, the little-endian encoding of
 *                     sum_i (y_i mod 2^d) 2^(i d): bit j of value i is stream bit i d + j, byte b holds stream bits 8b ... 8b + 7, least significant
 *                     first.  The unused high bits of a final partial byte are written as 0; no byte at or beyond nbytes is written.
 *   byte_decode       (ByteDecode_d, Algorithm 6): y_i = stream bits [i d, i d + d).  q = 0: written as they are, in [0, 2^d); q >= 2: written as
 *                     the least non-negative residue mod q (the m = q rule of ByteDecode_12), and *noncanonical is OR-ed with 1 if any value
 *                     was >= q (the modulus check of ML-KEM's encapsulation-key validation).  The flag may be NULL, is never cleared by the
 *                     call, and is never touched when q = 0.
 *   compress_encode   ByteEncode_d(Compress_d(x)), x read as its residue mod q;
 *   decode_decompress Decompress_d(ByteDecode_d(bytes)), the least non-negative residue.
 * For n d a multiple of 8 a flat call over several polynomials is the concatenation of their encodings (32 d bytes each at n = 256).
 * PSF_ERR_PARAM, in this order: d < 1; io_bits not 16 / 64; a NULL data pointer with len > 0; len d or a byte count that overflows size_t;
 * an output range that overlaps an input range (no in-place form); q = 1 in byte_decode; q < 2 in the two fused forms.  Then
 * PSF_ERR_UNSUPPORTED: d > 63; io_bits = 16 with d > 16 or q > 2^16; q >= 2^62.  len = 0 is PSF_OK.  Every check runs before the first HIP
 * call; nothing is launched or written on an error.  A valid call without a device is PSF_ERR_HIP (no CPU fallback).
 * Host forms: 64-bit words, allocate per call. */
psf_status psf_byte_encode(int device, uint32_t d, size_t len, const int64_t* y, uint8_t* bytes);
psf_status psf_byte_decode(int device, uint64_t q, uint32_t d, size_t len, const uint8_t* bytes, int64_t* y, int* noncanonical);
psf_status psf_compress_encode(int device, uint64_t q, uint32_t d, size_t len, const uint64_t* x, uint8_t* bytes);
psf_status psf_decode_decompress(int device, uint64_t q, uint32_t d, size_t len, const uint8_t* bytes, uint64_t* x);
/* The same on DEVICE buffers, ordered on `stream`, nothing allocated, never synchronising.  io_bits = 64: y int64 (read mod 2^d; written in
 * [0, 2^d) or [0, q)), x uint64; io_bits = 16: uint16 words, d <= 16, q <= 2^16.  d_noncanonical is a device int (or NULL).  Value buffers need
 * the alignment of their word, the byte buffer none; whole tiles (8192 16-bit or 2048 64-bit values) move by 16-byte vectors when both
 * pointers are 16-byte aligned, everything else byte by byte or value by value. */
psf_status psf_byte_encode_dev(int device, uint32_t d, size_t len, const void* d_y, uint8_t* d_bytes, int io_bits, void* stream);
psf_status psf_byte_decode_dev(int device, uint64_t q, uint32_t d, size_t len, const uint8_t* d_bytes, void* d_y, int* d_noncanonical, int io_bits, void* stream);
psf_status psf_compress_encode_dev(int device, uint64_t q, uint32_t d, size_t len, const void* d_x, uint8_t* d_bytes, int io_bits, void* stream);
psf_status psf_decode_decompress_dev(int device, uint64_t q, uint32_t d, size_t len, const uint8_t* d_bytes, void* d_x, int io_bits, void* stream);
/* Fills of `count` polynomials of n coefficients with samples (sample_uniform / sample_binomial / sample_discrete_gauss of MatZq,
 * PolynomialRingZq, MatPolynomialRingZq and MatZ: mp_perturbation.rs:222, trapdoor_distribution.rs, gadget_ring.rs), bound to no handle.
 * Layout: row-major, polynomial first_index + c at offset c n, constant term first.  Every value is a pure function of (seed, tag, global
 * polynomial index, coefficient), so filling [0, 8) equals filling [0, 3) and then [3, 8), bit for bit (DESIGN.md "Randomness contract").
 * `tag` selects the stream: 64 ... 255 are the caller's, 0 ... 63 belong to the library (PSF_ERR_PARAM); two tags under one seed are independent.
 * The tag word is tag | (index >> 32) << 8, so first_index + count <= 2^56, and the coefficient is a 32-bit counter word, so n < 2^32.
 *   uniform         on [0, q): multiply-shift with Lemire's rejection, attempt t from Philox block (i, (uint32)index, t, tag word) -- the rule of the
 *                   keys' a_bar.  Exact for 2 <= q < 2^62.  Words: uint64, or uint16 (io_bits = 16, q <= 2^16).
 *   cbd             centred binomial, 2 eta trials at p = 1/2 shifted by -eta (the law of FIPS 203's SamplePolyCBD_eta), 1 <= eta <= 16: with
 *                   s_w = floor(16 / eta), coefficient i is popcount(f & (2^eta - 1)) - popcount(f >> eta) of the 2 eta-bit field
 *                   f = (word >> 2 eta (i mod s_w)) & (2^(2 eta) - 1), word floor(i / s_w) mod 4 (x, y, z, w) of Philox block
 *                   (floor(i / (4 s_w)), (uint32)index, 0, tag word).  Words: int64 or int16 -- operand b of psf_matpoly_mul_*_dev.
 *   discrete_gauss  D_{Z,s,c} by the library's SampleZ (rejection from [ceil(c) - ceil(6 s), floor(c) + floor(6 s)], narrow or wide words by s
 *                   alone).  d_centers == NULL: the one centre `center` for the whole fill; otherwise count x n doubles, one centre per
 *                   coefficient (randomised rounding), and `center` is ignored.  Words: int64; int16 with a shared centre and
 *                   |center| + 6 s + 1 < 2^15.  A draw that ends at the cap of 65 536 attempts writes floor(c + 1/2), a centre with
 *                   |c| >= 2^62 writes 0; either ORs 1 into *d_fail (a device int, may be NULL, never cleared by the call), and the host form
 *                   returns PSF_ERR_SAMPLER.
 * Not offered: binomials with p != 1/2.  The SHAKE-derived, byte-exact SampleNTT / SamplePolyCBD of FIPS 203 are psf_sample_ntt_fips203* /
 * psf_sample_cbd_fips203* below (a different contract: their bits come from Keccak, not from the randomness contract of this library).
 * PSF_ERR_PARAM, in this order: tag outside 64 ... 255; io_bits not 16 / 64; n = 0 or n >= 2^32; first_index + count > 2^56 or a byte count that
 * overflows size_t; a NULL output pointer with count > 0; q < 2; eta = 0; s not finite or s <= 0; a shared centre that is not finite.  Then
 * PSF_ERR_UNSUPPORTED: q >= 2^62; io_bits = 16 with q > 2^16; eta > 16; s > 2^28 (the candidate count must fit 32 bits); io_bits = 16 with
 * per-element centres or a range that does not fit int16.  count = 0 is PSF_OK.  Every check runs before the first HIP call; nothing is launched
 * or written on an error.  A valid call without a device is PSF_ERR_HIP (no CPU fallback).
 * Device forms: ordered on `stream`, nothing allocated, never synchronising; the output needs the alignment of its word only. */
psf_status psf_sample_uniform_dev(int device, uint64_t seed, uint32_t tag, uint64_t first_index, size_t count, size_t n, uint64_t q, void* d_out, int io_bits,
                                  void* stream);
psf_status psf_sample_cbd_dev(int device, uint64_t seed, uint32_t tag, uint64_t first_index, size_t count, size_t n, uint32_t eta, void* d_out, int io_bits,
                              void* stream);
psf_status psf_sample_discrete_gauss_dev(int device, uint64_t seed, uint32_t tag, uint64_t first_index, size_t count, size_t n, double center,
                                         const double* d_centers, double s, void* d_out, int* d_fail, int io_bits, void* stream);
/* Host forms: 64-bit words, allocate per call, run on the device. */
psf_status psf_sample_uniform(int device, uint64_t seed, uint32_t tag, uint64_t first_index, size_t count, size_t n, uint64_t q, uint64_t* out);
psf_status psf_sample_cbd(int device, uint64_t seed, uint32_t tag, uint64_t first_index, size_t count, size_t n, uint32_t eta, int64_t* out);
psf_status psf_sample_discrete_gauss(int device, uint64_t seed, uint32_t tag, uint64_t first_index, size_t count, size_t n, double center,
                                     const double* centers, double s, int64_t* out);
/* FIPS 202 on the device: `count` independent messages of in_len bytes, message c at d_in + c * in_stride, digest c (out_len bytes) at
 * d_out + c * out_stride -- the functions H (SHA3-256), G (SHA3-512), J and PRF (SHAKE256) and XOF (SHAKE128) of FIPS 203, batched.  One Keccak
 * state per lane.  Any in_len (0 included; a message may take several absorb blocks) and, for the SHAKEs, any out_len >= 1 (several squeeze
 * blocks); out_len must be 32 for SHA3-256 and 64 for SHA3-512.  Pointers and strides need no alignment (8-byte groups move as one load or store
 * when base and stride are multiples of 8).
 * PSF_ERR_PARAM, in this order: unknown func; the wrong out_len for a SHA3; out_len = 0; a stride smaller than its length; a NULL pointer with
 * count > 0 (d_in may be NULL when in_len = 0); a byte count that overflows size_t; an output range that overlaps the input range.  count = 0 is
 * PSF_OK.  Every check runs before the first HIP call; nothing is launched or written on an error.  A valid call without a device is PSF_ERR_HIP
 * (no CPU fallback).  The device form is ordered on `stream`, allocates nothing and never synchronises; the host form allocates per call. */
enum { PSF_SHA3_256 = 0, PSF_SHA3_512 = 1, PSF_SHAKE128 = 2, PSF_SHAKE256 = 3 };
psf_status psf_keccak_dev(int device, int func, size_t count, const uint8_t* d_in, size_t in_len, size_t in_stride, uint8_t* d_out, size_t out_len,
                          size_t out_stride, void* stream);
psf_status psf_keccak(int device, int func, size_t count, const uint8_t* in, size_t in_len, size_t in_stride, uint8_t* out, size_t out_len, size_t out_stride);
/* FIPS 180-4 on the device, the twin of psf_keccak: `count` independent messages of in_len bytes, message c at d_in + c * in_stride, the leading
 * out_len bytes of digest c at d_out + c * out_stride (FIPS 205's Trunc) -- SHA-256 and SHA-512, what the SHA-2 parameter sets of SLH-DSA hash with.
 * One hash state per lane.  Any in_len (0 included; the padding opens a block of its own when it must); out_len is 1 ... 32 for SHA-256 and 1 ... 64
 * for SHA-512.  Pointers and strides need no alignment (4-byte groups of a message move as one load when base and stride are multiples of 4).
 * PSF_ERR_PARAM, in this order: unknown func; out_len = 0 or above the digest size; a stride smaller than its length; a NULL pointer with count > 0
 * (d_in may be NULL when in_len = 0); a byte count that overflows size_t; an output range that overlaps the input range.  count = 0 is PSF_OK.
 * Every check runs before the first HIP call; nothing is launched or written on an error.  A valid call without a device is PSF_ERR_HIP (no CPU
 * fallback).  The device form is ordered on `stream`, allocates nothing and never synchronises; the host form allocates per call. */
enum { PSF_SHA2_256 = 0, PSF_SHA2_512 = 1 };
psf_status psf_sha2_dev(int device, int func, size_t count, const uint8_t* d_in, size_t in_len, size_t in_stride, uint8_t* d_out, size_t out_len,
                        size_t out_stride, void* stream);
psf_status psf_sha2(int device, int func, size_t count, const uint8_t* in, size_t in_len, size_t in_stride, uint8_t* out, size_t out_len, size_t out_stride);
/* The byte-exact samplers of FIPS 203 (q = 3329, n = 256), one polynomial per lane, 256 coefficients per polynomial, polynomials contiguous.
 *   sample_ntt  SampleNTT (Algorithm 7): coefficients in [0, q) in the order the algorithm produces them -- FIPS 203's NTT-domain representation
 *               (psf_ntt_image_from_fips203_dev makes it an operand of the *_hat_dev products).  Words: uint16 or uint64 (operand a).
 *               k = 0, the raw form: input c is the 34 bytes at d_seed + c * seed_stride, output polynomial c.
 *               1 <= k <= 16, the matrix form: input c is a 32-byte rho_c; the output is count * k * k polynomials, polynomial (c, i, j), row-major,
 *               = SampleNTT(rho_c || byte(j) || byte(i)): A_hat[i][j] of K-PKE.KeyGen, the rows = inner = k operand A of batch c.
 *               The squeeze loop is capped at 8 SHAKE128 blocks (the standard's loop is unbounded; more than 6 are needed with probability below
 *               2^-440): a polynomial that reaches the cap gets zeros for its remaining coefficients and ORs 1 into *d_fail (a device int, may be
 *               NULL, never cleared by the call); the host form returns PSF_ERR_SAMPLER.
 *   sample_cbd  SamplePolyCBD_eta(PRF_eta(sigma, N)) (Algorithm 8, PRF_eta(sigma, N) = SHAKE256(sigma || byte(N), 64 eta)): `count` 32-byte seeds
 *               sigma_c at d_sigma + c * sigma_stride; polynomial (c, t), t < per_seed, uses N = first_nonce + t; count * per_seed polynomials of
 *               signed coefficients in [-eta, eta].  Words: int16 or int64 (operand b and the addend E).
 * PSF_ERR_PARAM, in this order: k > 16; eta = 0; first_nonce + per_seed > 256; io_bits not 16 / 64; a stride smaller than the seed; a NULL seed or
 * output pointer with count > 0; a byte count that overflows size_t; an output range that overlaps the seeds.  Then PSF_ERR_UNSUPPORTED: eta other
 * than 2 or 3.  count = 0 (or per_seed = 0) is PSF_OK.  Every check runs before the first HIP call; nothing is launched or written on an error.  A
 * valid call without a device is PSF_ERR_HIP.  Device forms: ordered on `stream`, nothing allocated, never synchronising; seeds need no alignment,
 * the output that of its word.  Host forms: 64-bit words, allocate per call, run on the device. */
psf_status psf_sample_ntt_fips203_dev(int device, size_t count, uint32_t k, const uint8_t* d_seed, size_t seed_stride, void* d_out, int* d_fail, int io_bits,
                                      void* stream);
psf_status psf_sample_cbd_fips203_dev(int device, size_t count, uint32_t eta, const uint8_t* d_sigma, size_t sigma_stride, uint32_t first_nonce, uint32_t per_seed,
                                      void* d_out, int io_bits, void* stream);
psf_status psf_sample_ntt_fips203(int device, size_t count, uint32_t k, const uint8_t* seed, size_t seed_stride, uint64_t* out);
psf_status psf_sample_cbd_fips203(int device, size_t count, uint32_t eta, const uint8_t* sigma, size_t sigma_stride, uint32_t first_nonce, uint32_t per_seed,
                                  int64_t* out);
/* NTT-domain interop at q = 3329, n = 256, the ring X^n + 1: FIPS 203 keeps A_hat, t_hat and s_hat in the NTT domain (an encapsulation key is
 * ByteEncode_12(t_hat) || rho).  `from` reads `count` polynomials in FIPS 203's representation (uint16 in [0, q), or uint64 of any value read mod q)
 * and writes images (count * 256 32-bit words) that every negacyclic *_hat_dev product accepts at (3329, 256), with exactly the results of the
 * coefficient-domain polynomial NTT^-1(f_hat) of Algorithm 10.  `to` reads images written by psf_ntt_forward_dev or by `from` and writes canonical
 * residues in [0, q): for an image of f, the output of Algorithm 9 on f.  Both representations hold the residues of f modulo the same 128 quadratic
 * factors; the conversion is a fixed permutation of the factors and a change of scale.  Images of the cyclic ring and of other (q, n) have no such form.
 * PSF_ERR_PARAM: io_bits not 16 / 64, a NULL pointer with count > 0, a byte count that overflows size_t, overlapping buffers.  count = 0 is PSF_OK.
 * Checks before the first HIP call, PSF_ERR_HIP without a device.  Device forms: ordered on `stream`, nothing allocated.  Host forms: 64-bit words. */
psf_status psf_ntt_image_from_fips203_dev(int device, size_t count, const void* d_fhat, int io_bits, uint32_t* d_hat, void* stream);
psf_status psf_ntt_image_to_fips203_dev(int device, size_t count, const uint32_t* d_hat, void* d_fhat, int io_bits, void* stream);
psf_status psf_ntt_image_from_fips203(int device, size_t count, const uint64_t* fhat, uint32_t* hat);
psf_status psf_ntt_image_to_fips203(int device, size_t count, const uint32_t* hat, uint64_t* fhat);
/* ML-KEM (FIPS 203), batched, bytes in and bytes out.  The library draws NO randomness here: d, z and m are the caller's 32-byte strings, and the
 * algorithms offered are the "internal" ones -- ML-KEM.KeyGen_internal(d, z) (Algorithm 16), ML-KEM.Encaps_internal(ek, m) (Algorithm 17) and
 * ML-KEM.Decaps_internal(dk, c) (Algorithm 18) -- which is what makes every output a function of the inputs that a test can compare.  A caller
 * implements Algorithms 19 to 21 by drawing d, z and m from an approved random-bit generator and running the two input checks below first
 * (INTEGRATION.md).  The value of a parameter set is its k; (eta1, eta2, du, dv) = (3, 2, 10, 4), (2, 2, 10, 4), (2, 2, 11, 5).
 *   sizes in bytes:  ek 384 k + 32 (800 / 1184 / 1568), dk 768 k + 96 (1632 / 2400 / 3168), ct 32 (du k + dv) (768 / 1088 / 1568), ss 32.
 * Batches are contiguous: instance c of a buffer is at base + c * size.  Type checks are implicit in these fixed sizes.
 *   keygen   (rho, sigma) = G(d || byte(k)); (ek, dk_pke) = K-PKE.KeyGen; dk = dk_pke || ek || H(ek) || z.
 *   encaps   (K, r) = G(m || H(ek)); c = K-PKE.Encrypt(ek, m, r).  ss = K.
 *   decaps   m' = K-PKE.Decrypt(dk[0 : 384 k], c); (K', r') = G(m' || dk[768 k + 32 : 768 k + 64]); K_bar = J(dk[768 k + 64 : 768 k + 96] || c);
 *            c' = K-PKE.Encrypt(dk[384 k : 768 k + 32], m', r'); ss = K' if c = c', else K_bar.  The comparison reads every byte of c and c', K_bar
 *            is always computed, and the selection is mask arithmetic: nothing in this layer branches on secret data (SampleNTT's rejection loop
 *            runs on the public rho only).
 *   check_ek the modulus check of section 7.2: ok[c] = 1 exactly when every 12-bit field of ek_c[0 : 384 k] is below q, else 0.
 *   check_dk the hash check of section 7.3: ok[c] = 1 exactly when H(dk_c[384 k : 768 k + 32]) = dk_c[768 k + 32 : 768 k + 64], else 0.
 * psf_mlkem_workspace_bytes gives the bytes of d_ws an operation needs for `count` instances (op: keygen / encaps / decaps / check; 0 for check): a
 * multiple of 256, monotone in count.  Secret intermediates (s, e, y, e1, e2, m', r', K', the images of the secret key) exist only there, and the
 * last thing each entry point queues on `stream` sets those bytes of d_ws to zero.
 * Device forms: ordered on `stream`, nothing allocated, never synchronising.  Byte buffers need no alignment; d_ws must be 256-byte aligned.
 * d_fail is a device int (may be NULL, never cleared by the call), OR-ed with 1 when a SampleNTT reaches its cap of 8 blocks.
 * PSF_ERR_PARAM, in this order: an unknown param (or op); a NULL data pointer with count > 0; a byte count that overflows size_t; d_ws NULL or
 * misaligned, or ws_bytes below the required size; an output range that overlaps an input, another output or the workspace.  count = 0 is PSF_OK.
 * More than 2^31 - 1 instances in one call is PSF_ERR_UNSUPPORTED.  Every check runs before the first HIP call; nothing is launched or written on an
 * error.  A valid call without a device is PSF_ERR_HIP (no CPU fallback).
 * Host forms: the same arguments without workspace, flag and stream; they allocate per call, run on the device and return PSF_ERR_SAMPLER if the
 * flag was raised. */
enum { PSF_MLKEM_512 = 2, PSF_MLKEM_768 = 3, PSF_MLKEM_1024 = 4 };
enum { PSF_MLKEM_OP_KEYGEN = 0, PSF_MLKEM_OP_ENCAPS = 1, PSF_MLKEM_OP_DECAPS = 2, PSF_MLKEM_OP_CHECK = 3 };
psf_status psf_mlkem_sizes(int param, size_t* ek, size_t* dk, size_t* ct, size_t* ss);
psf_status psf_mlkem_workspace_bytes(int param, size_t count, int op, size_t* bytes);
psf_status psf_mlkem_keygen_dev(int device, int param, size_t count, const uint8_t* d_d, const uint8_t* d_z, uint8_t* d_ek, uint8_t* d_dk, void* d_ws, size_t ws_bytes,
                                int* d_fail, void* stream);
psf_status psf_mlkem_encaps_dev(int device, int param, size_t count, const uint8_t* d_ek, const uint8_t* d_m, uint8_t* d_ss, uint8_t* d_ct, void* d_ws, size_t ws_bytes,
                                int* d_fail, void* stream);
psf_status psf_mlkem_decaps_dev(int device, int param, size_t count, const uint8_t* d_dk, const uint8_t* d_ct, uint8_t* d_ss, void* d_ws, size_t ws_bytes, int* d_fail,
                                void* stream);
psf_status psf_mlkem_check_ek_dev(int device, int param, size_t count, const uint8_t* d_ek, uint8_t* d_ok, void* stream);
psf_status psf_mlkem_check_dk_dev(int device, int param, size_t count, const uint8_t* d_dk, uint8_t* d_ok, void* stream);
psf_status psf_mlkem_keygen(int device, int param, size_t count, const uint8_t* d, const uint8_t* z, uint8_t* ek, uint8_t* dk);
psf_status psf_mlkem_encaps(int device, int param, size_t count, const uint8_t* ek, const uint8_t* m, uint8_t* ss, uint8_t* ct);
psf_status psf_mlkem_decaps(int device, int param, size_t count, const uint8_t* dk, const uint8_t* ct, uint8_t* ss);
psf_status psf_mlkem_check_ek(int device, int param, size_t count, const uint8_t* ek, uint8_t* ok);
psf_status psf_mlkem_check_dk(int device, int param, size_t count, const uint8_t* dk, uint8_t* ok);
/* ML-DSA (FIPS 204, August 2024), batched, bytes in and bytes out: ML-DSA.KeyGen_internal(xi) (Algorithm 6) and ML-DSA.Verify_internal(pk, M', sigma)
 * (Algorithm 8) for ML-DSA-44, -65 and -87; signing (Algorithm 7) is psf_mldsa_sign_* below.  The library draws NO randomness: xi is the caller's 32-byte string.  The value
 * of a parameter set is its number; (k, l, eta, tau, lambda / 4, gamma1, gamma2, beta, omega) = (4, 4, 2, 39, 32, 2^17, (q - 1) / 88, 78, 80),
 * (6, 5, 4, 49, 48, 2^19, (q - 1) / 32, 196, 55), (8, 7, 2, 60, 64, 2^19, (q - 1) / 32, 120, 75); q = 8380417, n = 256, d = 13.
 *   sizes in bytes:  pk 32 + 320 k (1312 / 1952 / 2592), sk 128 + 32 ((k + l) bitlen(2 eta) + 13 k) (2560 / 4032 / 4896),
 *                    sig lambda / 4 + 32 l (1 + bitlen(gamma1 - 1)) + omega + k (2420 / 3309 / 4627).
 *   keygen   (rho, rho', K) = H(xi || byte(k) || byte(l), 128); A_hat = ExpandA(rho); (s1, s2) = ExpandS(rho'); t = NTT^-1(A_hat o NTT(s1)) + s2;
 *            (t1, t0) = Power2Round(t); pk = pkEncode(rho, t1); tr = H(pk, 64); sk = skEncode(rho, K, tr, s1, s2, t0).  xi, pk and sk are contiguous:
 *            instance c at base + c * size.  rho', s1, s2, t, t0 and the images of A_hat exist only in d_ws (K goes straight into sk), and the last
 *            thing the call queues on `stream` sets those bytes of d_ws to zero.
 *   verify   Algorithm 8.  Key c is at d_pk + c * pk_stride; pk_stride = 0 means one key for all instances (A_hat and tr are then formed once),
 *            otherwise pk_stride >= the pk size.  Messages have one length per call: instance c's msg_len bytes are at d_msg + c * msg_stride.
 *            msg_kind = PSF_MLDSA_MSG_BYTES: the bytes are M' and mu = H(tr || M', 64) -- the caller formats M' = 0 || |ctx| || ctx || M for
 *            Algorithm 3; PSF_MLDSA_MSG_MU: msg_len must be 64, the bytes are mu itself, and tr is not computed.  Signatures are contiguous.
 *            d_ok[c] is 1 or 0.  d_why (may be NULL) gets an OR of
 *              PSF_MLDSA_WHY_HINT  HintBitUnpack returns bottom: a count byte below the running index or above omega, indices inside one polynomial
 *                                  not strictly increasing, or a non-zero byte after the last index;
 *              PSF_MLDSA_WHY_NORM  ||z||_inf >= gamma1 - beta, evaluated from the signature bytes whatever the hint says;
 *              PSF_MLDSA_WHY_HASH  c~' != c~; also set whenever WHY_HINT is, and no w1' is formed from a malformed hint;
 *            and ok = (why == 0).  Nothing in verification is secret: its workspace is NOT cleared and needs no clearing.
 * psf_mldsa_workspace_bytes gives the bytes of d_ws an operation needs for `count` instances (op: keygen / verify): a multiple of 256, monotone in
 * count; the verify size serves every pk_stride.  d_ws holds: keygen rho' | images of A_hat | s1 | s2 | t; verify tr | mu | the why words | the hint
 * masks | images of A_hat | z | t1 2^d | c | w'.  Polynomials are 64-bit words there (2 KiB each), images 1 KiB.
 * Device forms: ordered on `stream`, nothing allocated, never synchronising.  Byte buffers need no alignment; d_ws must be 256-byte aligned.
 * d_fail is a device int (may be NULL, never cleared by the call), OR-ed with 1 when a sampler reaches its cap of 8 blocks; the sampler then leaves
 * zeros for what is missing.  With acceptance rate p per candidate a cap is reached when fewer than 256 (SampleInBall: tau) of the candidates of 8
 * blocks are accepted, bounded by exp(-m D(256 / m || p)): RejNTTPoly (m = 448 candidates of 3 bytes, p = q / 2^23) below 2^-1479; RejBoundedPoly
 * (m = 2176 half bytes) below 2^-6566 at p = 15 / 16 (eta = 2) and below 2^-1365 at p = 9 / 16 (eta = 4); SampleInBall (1080 bytes for at most 64
 * draws, draw i accepted with (i + 1) / 256 >= 3 / 4) below 2^-1708.
 * PSF_ERR_PARAM, in this order: an unknown param, op or msg_kind; a NULL data pointer with count > 0 (d_msg may be NULL when msg_len = 0, d_why
 * always); a stride below its length (except pk_stride = 0), or PSF_MLDSA_MSG_MU with msg_len != 64; a byte count that overflows size_t; d_ws NULL or
 * misaligned, or ws_bytes below the required size; an output range that overlaps an input, another output or the workspace.  Then
 * PSF_ERR_UNSUPPORTED for more than 2^31 - 1 instances.  count = 0 is PSF_OK.  Every check runs before the first HIP call; nothing is launched or
 * written on an error.  A valid call without a device is PSF_ERR_HIP (no CPU fallback).
 * Host forms: the same arguments without workspace, flag and stream; they allocate per call, run on the device and return PSF_ERR_SAMPLER if the
 * flag was raised. */
enum { PSF_MLDSA_44 = 44, PSF_MLDSA_65 = 65, PSF_MLDSA_87 = 87 };
enum { PSF_MLDSA_OP_KEYGEN = 0, PSF_MLDSA_OP_VERIFY = 1 };
enum { PSF_MLDSA_MSG_BYTES = 0, PSF_MLDSA_MSG_MU = 1 };
enum { PSF_MLDSA_WHY_HINT = 1, PSF_MLDSA_WHY_NORM = 2, PSF_MLDSA_WHY_HASH = 4 };
psf_status psf_mldsa_sizes(int param, size_t* pk, size_t* sk, size_t* sig);
psf_status psf_mldsa_workspace_bytes(int param, size_t count, int op, size_t* bytes);
psf_status psf_mldsa_keygen_dev(int device, int param, size_t count, const uint8_t* d_xi, uint8_t* d_pk, uint8_t* d_sk, void* d_ws, size_t ws_bytes, int* d_fail,
                                void* stream);
psf_status psf_mldsa_verify_dev(int device, int param, size_t count, const uint8_t* d_pk, size_t pk_stride, const uint8_t* d_msg, size_t msg_len, size_t msg_stride,
                                int msg_kind, const uint8_t* d_sig, uint8_t* d_ok, uint8_t* d_why, void* d_ws, size_t ws_bytes, int* d_fail, void* stream);
psf_status psf_mldsa_keygen(int device, int param, size_t count, const uint8_t* xi, uint8_t* pk, uint8_t* sk);
psf_status psf_mldsa_verify(int device, int param, size_t count, const uint8_t* pk, size_t pk_stride, const uint8_t* msg, size_t msg_len, size_t msg_stride,
                            int msg_kind, const uint8_t* sig, uint8_t* ok, uint8_t* why);
/* ML-DSA.Sign_internal(sk, M', rnd) (Algorithm 7), batched: sigma_c for `count` instances, one key for all (sk_stride = 0) or key c at
 * d_sk + c * sk_stride (sk_stride >= the sk size).  The rejection loop is three device calls, none of which synchronises, and one number that the
 * caller carries between them:
 *   begin   fills slot j of the workspace with instance j: the images of s1, s2, t0 (skDecode, NTT) and of A_hat = ExpandA(rho); mu = H(tr || M', 64)
 *           with tr read from sk (msg_kind, msg_len and msg_stride as in verify; PSF_MLDSA_MSG_MU: the 64 message bytes are mu);
 *           rho'' = H(K || rnd || mu, 64) with rnd the 32 bytes at d_rnd + 32 c, or 32 zero bytes when d_rnd is NULL (the deterministic variant; the
 *           library draws no randomness); kappa = 0.  It writes `count` to the device word *d_live.
 *   round   one attempt for the instances in the first m = min(active, *d_live) slots: y = ExpandMask(rho'', kappa), kappa += l, w = A y,
 *           c~ = H(mu || w1Encode(HighBits(w)), lambda / 4), c = SampleInBall(c~), z = y + c s1, r = w - c s2, and the four tests ||z|| >= gamma1 - beta,
 *           ||LowBits(r)|| >= gamma2 - beta, ||c t0|| >= gamma2, more than omega ones in MakeHint(-c t0, r + c t0).  An accepted instance gets
 *           sigEncode(c~, z mod+- q, h) at d_sig + index * sig size and its number of attempts at d_rounds[index] (d_rounds may be NULL), and leaves
 *           the live set; a rejected one writes nothing outside the workspace.  Then the live slots are made dense again, [0, new_live): holes of
 *           the new prefix are filled from live slots beyond it, and new_live is written to *d_live.  `active` is a host value in [0, count] that
 *           sizes the launches; the kernels read *d_live and skip slots at or beyond it, so any `active` is safe: a smaller one than *d_live leaves
 *           some instances unattempted in this round, a larger one costs product work on dead slots.  A signature is a function of (sk, mu, rnd)
 *           alone: not of the schedule of `active`, the batch or the slot.  An instance whose counter is used up (kappa + l > 2^16 before an
 *           attempt; probability below 0.8^9000) is retired unsigned and d_fail is OR-ed with 2.
 *   end     sets every byte of the workspace to zero: everything in it but A_hat is secret.  Call it whether or not every instance was signed.
 * The caller reads *d_live (4 bytes) when it chooses to, passes it as the next `active`, and stops at 0.  count, sk_stride, d_ws and d_live are the
 * same in every call of one signing.
 * psf_mldsa_sign_workspace_bytes: the bytes of d_ws for `count` instances, a multiple of 256, monotone in count, smaller for sk_stride = 0.  d_ws
 * holds the images of A_hat (k l KiB) | s1_hat | s2_hat | t0_hat (l + 2 k KiB) -- per slot, or once when sk_stride = 0 -- then per slot mu | rho'' |
 * kappa | index, the control words, and the per-round scratch y | w (then r) | c | z | c t0 | c~ | flags | holes | sources (64-bit words, 2 KiB a
 * polynomial), which is never moved.
 * PSF_ERR_PARAM, in this order: an unknown param or msg_kind (host form: max_rounds < 1 or max_rounds * l > 65536); a NULL d_sk, d_msg (unless
 * msg_len = 0), d_sig or d_live with count > 0 (d_rnd and d_rounds may be NULL); sk_stride neither 0 nor >= the sk size, msg_stride < msg_len,
 * PSF_MLDSA_MSG_MU with msg_len != 64, active > count; a byte count that overflows size_t; d_ws NULL, misaligned (256) or ws_bytes too small; d_live
 * or d_rounds not 4-byte aligned; an output (d_live, d_sig, d_rounds) that overlaps an input, another output or the workspace.  Then
 * PSF_ERR_UNSUPPORTED above 2^31 - 1 instances.  count = 0 is PSF_OK.  Every check runs before the first HIP call; a valid call without a device is
 * PSF_ERR_HIP.  d_fail as above (1: a sampler cap; 2: a counter used up).
 * Host form psf_mldsa_sign: allocates, zero-fills sig (and rounds, which may be NULL), runs begin, then rounds with active = the 4 bytes of d_live read
 * back after each, until it is 0 or max_rounds rounds have run, then end.  PSF_ERR_SAMPLER if instances remain or the flag was raised: their sig
 * stays zero and their rounds[c] is 0. */
psf_status psf_mldsa_sign_workspace_bytes(int param, size_t count, size_t sk_stride, size_t* bytes);
psf_status psf_mldsa_sign_begin_dev(int device, int param, size_t count, const uint8_t* d_sk, size_t sk_stride, const uint8_t* d_msg, size_t msg_len,
                                    size_t msg_stride, int msg_kind, const uint8_t* d_rnd, void* d_ws, size_t ws_bytes, uint32_t* d_live, int* d_fail, void* stream);
psf_status psf_mldsa_sign_round_dev(int device, int param, size_t count, size_t sk_stride, size_t active, uint8_t* d_sig, uint32_t* d_rounds, void* d_ws,
                                    size_t ws_bytes, uint32_t* d_live, int* d_fail, void* stream);
psf_status psf_mldsa_sign_end_dev(int device, int param, size_t count, size_t sk_stride, void* d_ws, size_t ws_bytes, void* stream);
psf_status psf_mldsa_sign(int device, int param, size_t count, const uint8_t* sk, size_t sk_stride, const uint8_t* msg, size_t msg_len, size_t msg_stride,
                          int msg_kind, const uint8_t* rnd, uint8_t* sig, uint32_t max_rounds, uint32_t* rounds);
/* The stages of ML-DSA as entry points of their own: 64-bit words, one polynomial of 256 coefficients per lane, polynomials contiguous.
 *   sample_ntt      RejNTTPoly (Algorithm 30): coefficients in [0, q) in FIPS 204's NTT-domain order.  k = l = 0, the raw form: input c is the 34
 *                   bytes at d_seed + c * seed_stride, output polynomial c.  Otherwise (1 <= k, l <= 255) input c is a 32-byte rho_c and the output is
 *                   count * k * l polynomials; polynomial (c, r, s), row-major, is RejNTTPoly(rho_c || byte(s) || byte(r)): A_hat of ExpandA, operand A
 *                   of batch c with rows = k and inner = l once psf_ntt_image_from_fips204_dev has made images of it.
 *   sample_bounded  RejBoundedPoly (Algorithm 31): polynomial (c, t), t < per_seed, is RejBoundedPoly(seed_c || le16(first_nonce + t)) from the
 *                   64-byte seed at d_seed + c * seed_stride; signed coefficients in [-eta, eta].  first_nonce + per_seed <= 65536.
 *   sample_in_ball  SampleInBall (Algorithm 29) of the ctilde_len bytes at d_ctilde + c * ctilde_stride, 1 <= tau <= 64: coefficients in {-1, 0, 1}.
 *   image_from      reads `count` polynomials as Algorithm 41 (NTT) leaves them, any 64-bit value read mod q, and writes images (count * 256 32-bit
 *                   words) that every negacyclic *_hat_dev product accepts at (8380417, 256).  A fixed permutation and a change of scale, as its
 *                   FIPS 203 twin is.  There is no `to` direction: no ML-DSA key or signature holds an NTT-domain value.
 * d_fail and the cap of 8 blocks are those of the ML-DSA entry points above.
 * PSF_ERR_PARAM, in this order: k or l above 255, or exactly one of them 0; eta = 0; first_nonce + per_seed > 65536; tau outside [1, 64]; a stride
 * smaller than the seed; a NULL seed or output pointer with count > 0; a byte count that overflows size_t; an output range that overlaps the seeds.
 * Then PSF_ERR_UNSUPPORTED: eta other than 2 or 4.  count = 0 (or per_seed = 0) is PSF_OK.  Every check runs before the first HIP call; nothing is
 * launched or written on an error.  A valid call without a device is PSF_ERR_HIP.  Device forms: ordered on `stream`, nothing allocated, never
 * synchronising; seeds need no alignment, the output that of its word.  Host forms: allocate per call, run on the device, PSF_ERR_SAMPLER if the
 * flag was raised. */
psf_status psf_sample_ntt_fips204_dev(int device, size_t count, uint32_t k, uint32_t l, const uint8_t* d_seed, size_t seed_stride, uint64_t* d_out, int* d_fail,
                                      void* stream);
psf_status psf_sample_bounded_fips204_dev(int device, size_t count, uint32_t eta, const uint8_t* d_seed, size_t seed_stride, uint32_t first_nonce, uint32_t per_seed,
                                          int64_t* d_out, int* d_fail, void* stream);
psf_status psf_sample_in_ball_fips204_dev(int device, size_t count, uint32_t tau, const uint8_t* d_ctilde, size_t ctilde_len, size_t ctilde_stride, int64_t* d_out,
                                          int* d_fail, void* stream);
psf_status psf_ntt_image_from_fips204_dev(int device, size_t count, const uint64_t* d_fhat, uint32_t* d_hat, void* stream);
psf_status psf_sample_ntt_fips204(int device, size_t count, uint32_t k, uint32_t l, const uint8_t* seed, size_t seed_stride, uint64_t* out);
psf_status psf_sample_bounded_fips204(int device, size_t count, uint32_t eta, const uint8_t* seed, size_t seed_stride, uint32_t first_nonce, uint32_t per_seed,
                                      int64_t* out);
psf_status psf_sample_in_ball_fips204(int device, size_t count, uint32_t tau, const uint8_t* ctilde, size_t ctilde_len, size_t ctilde_stride, int64_t* out);
psf_status psf_ntt_image_from_fips204(int device, size_t count, const uint64_t* fhat, uint32_t* hat);
/* SLH-DSA (FIPS 205, August 2024), batched, bytes in and bytes out: slh_keygen_internal(SK.seed, SK.prf, PK.seed) (Algorithm 18) and
 * slh_verify_internal(M, SIG, PK) (Algorithm 20) and slh_sign_internal(M, SK, addrnd) (Algorithm 19, below) for the six SHAKE parameter sets.  KeyGen and Verify
 * and signing of the six SHA-2 sets are psf_slhdsa_sha2_* (below, a parameter numbering of their own); HashSLH-DSA is not here.  The library draws NO randomness: the three seeds and addrnd are the caller's n-byte strings.  (n, h, d, h', a, k, m) = 128s (16, 63, 7, 9, 12, 14, 30), 128f (16, 66, 22, 3, 6, 33, 34),
 * 192s (24, 63, 7, 9, 14, 17, 39), 192f (24, 66, 22, 3, 8, 33, 42), 256s (32, 64, 8, 8, 14, 22, 47), 256f (32, 68, 17, 4, 9, 35, 49); lg_w = 4,
 * len = 2 n + 3.  The hash functions are those of section 11.1, all SHAKE256: H_msg = SHAKE256(R || PK.seed || PK.root || M, 8 m), PRF, F, H and
 * T_l = SHAKE256(PK.seed || ADRS || ..., 8 n) with the uncompressed 32-byte ADRS.
 *   sizes in bytes:  pk 2 n (32 / 48 / 64), sk 4 n (64 / 96 / 128), sig (1 + k (1 + a) + h + d len) n (7856 / 17088 / 16224 / 35664 / 29792 / 49856).
 *   keygen   PK.root = xmss_node(SK.seed, 0, h', PK.seed, ADRS{layer d - 1, tree 0}); pk = PK.seed || PK.root, sk = SK.seed || SK.prf || PK.seed ||
 *            PK.root.  The three inputs, pk and sk are contiguous: instance c at base + c * size.  The WOTS+ secret values and the chain intermediates
 *            exist in registers only; every chain runs its 15 steps; no branch and no address depends on a secret.  d_ws receives the chain ends and
 *            the leaves (public values), and the last thing the call queues on `stream` sets every byte of d_ws to zero.
 *   verify   Algorithm 20.  Key c is at d_pk + c * pk_stride; pk_stride = 0 means one key for all instances, otherwise pk_stride >= 2 n.  Messages
 *            have one length per call: instance c's msg_len bytes are at d_msg + c * msg_stride.  The bytes are the M of Algorithm 20 -- the caller
 *            formats M' = 0 || |ctx| || ctx || M for Algorithm 24.  Signatures are contiguous, at the fixed size.  d_ok[c] is 1 or 0.  Nothing in
 *            verification is secret: its workspace is NOT cleared and needs no clearing.
 * psf_slhdsa_workspace_bytes gives the bytes of d_ws an operation needs for `count` instances (op: keygen / verify): a multiple of 256, monotone in
 * count; the verify size serves every pk_stride.  d_ws holds: keygen the chain ends (2^h' len n bytes per instance) | the leaves (2^h' n); verify the
 * first 64 bytes of H_msg | the k FORS roots | the current node (32 bytes) | the len chain ends of the current layer.
 * Device forms: ordered on `stream`, nothing allocated, never synchronising.  Byte buffers need no alignment; d_ws must be 256-byte aligned.
 * PSF_ERR_PARAM, in this order: an unknown param or op; a NULL data pointer with count > 0 (d_msg may be NULL when msg_len = 0); a stride below its
 * length (except pk_stride = 0); a byte count that overflows size_t; d_ws NULL or misaligned, or ws_bytes below the required size; an output range
 * that overlaps an input, another output or the workspace.  Then PSF_ERR_UNSUPPORTED for more than 2^31 - 1 instances.  count = 0 is PSF_OK.  Every
 * check runs before the first HIP call; nothing is launched or written on an error.  A valid call without a device is PSF_ERR_HIP (no CPU fallback).
 * Host forms: the same arguments without workspace and stream; they allocate per call and run on the device.
 *   sign     Algorithm 19, byte-identical to the standard's pseudocode.  Key c is the 4 n bytes at d_sk + c * sk_stride; sk_stride = 0 means one key for
 *            all instances, otherwise sk_stride >= 4 n.  Messages as in verify: one length per call, instance c's msg_len bytes at d_msg + c *
 *            msg_stride, the bytes are the M of Algorithm 19 (the caller formats M' = 0 || |ctx| || ctx || M for Algorithm 22); d_msg may be NULL when
 *            msg_len = 0.  d_addrnd is NULL -- the deterministic variant, opt_rand = PK.seed read from the key -- or n bytes per instance, contiguous:
 *            instance c uses the n bytes at d_addrnd + c * n.  Signatures are contiguous at the fixed size.  A signature is a function of (sk, M,
 *            addrnd) alone: not of the batch, the position in it or sk_stride.  No WOTS+ or FORS secret value and no chain intermediate is stored to
 *            memory except the ones that ARE the signature; no branch, loop bound or address depends on a secret (indices and digits come from the
 *            digest and from roots, which a verifier recomputes).
 * psf_slhdsa_sign_workspace_bytes gives the bytes of d_ws for `count` instances: a multiple of 256, monotone in count, 0 for count = 0, the same for
 * every sk_stride.  d_ws holds, each section rounded up to 256 bytes: the first 64 bytes of H_msg per instance | the FORS subtree roots (k 2^(a - 9) n
 * bytes per instance when a > 9, else nothing) | the k FORS roots (k n) | the messages of the d layers (32 d) | the chain ends of all d trees
 * (d 2^h' len n) | their leaves (d 2^h' n): public values only.  The device form is ordered on `stream`, allocates nothing and never synchronises;
 * byte buffers need no alignment, d_ws must be 256-byte aligned; the last thing the call queues on `stream` sets every byte of d_ws to zero.
 * PSF_ERR_PARAM, in this order: an unknown param (psf_slhdsa_sign_workspace_bytes: also a NULL `bytes`); a NULL d_sk, d_msg (unless msg_len = 0) or
 * d_sig with count > 0; sk_stride neither 0 nor >= 4 n, or msg_stride < msg_len; a byte count that overflows size_t; d_ws NULL or misaligned, or
 * ws_bytes too small; d_sig overlapping an input or the workspace.  Then PSF_ERR_UNSUPPORTED above 2^31 - 1 instances.  count = 0 is PSF_OK after the
 * param check.  Every check runs before the first HIP call; nothing is launched or written on an error.  A valid call without a device is PSF_ERR_HIP.
 * Host form psf_slhdsa_sign: the same arguments without workspace and stream; it allocates per call, runs on the device and zeroes its device copies
 * of sk and addrnd before freeing them. */
enum { PSF_SLHDSA_SHAKE_128S = 0, PSF_SLHDSA_SHAKE_128F = 1, PSF_SLHDSA_SHAKE_192S = 2, PSF_SLHDSA_SHAKE_192F = 3, PSF_SLHDSA_SHAKE_256S = 4,
       PSF_SLHDSA_SHAKE_256F = 5 };
enum { PSF_SLHDSA_OP_KEYGEN = 0, PSF_SLHDSA_OP_VERIFY = 1 };
psf_status psf_slhdsa_sizes(int param, size_t* pk, size_t* sk, size_t* sig);
psf_status psf_slhdsa_workspace_bytes(int param, size_t count, int op, size_t* bytes);
psf_status psf_slhdsa_keygen_dev(int device, int param, size_t count, const uint8_t* d_sk_seed, const uint8_t* d_sk_prf, const uint8_t* d_pk_seed, uint8_t* d_pk,
                                 uint8_t* d_sk, void* d_ws, size_t ws_bytes, void* stream);
psf_status psf_slhdsa_verify_dev(int device, int param, size_t count, const uint8_t* d_pk, size_t pk_stride, const uint8_t* d_msg, size_t msg_len, size_t msg_stride,
                                 const uint8_t* d_sig, uint8_t* d_ok, void* d_ws, size_t ws_bytes, void* stream);
psf_status psf_slhdsa_keygen(int device, int param, size_t count, const uint8_t* sk_seed, const uint8_t* sk_prf, const uint8_t* pk_seed, uint8_t* pk, uint8_t* sk);
psf_status psf_slhdsa_verify(int device, int param, size_t count, const uint8_t* pk, size_t pk_stride, const uint8_t* msg, size_t msg_len, size_t msg_stride,
                             const uint8_t* sig, uint8_t* ok);
psf_status psf_slhdsa_sign_workspace_bytes(int param, size_t count, size_t* bytes);
psf_status psf_slhdsa_sign_dev(int device, int param, size_t count, const uint8_t* d_sk, size_t sk_stride, const uint8_t* d_msg, size_t msg_len, size_t msg_stride,
                               const uint8_t* d_addrnd, uint8_t* d_sig, void* d_ws, size_t ws_bytes, void* stream);
psf_status psf_slhdsa_sign(int device, int param, size_t count, const uint8_t* sk, size_t sk_stride, const uint8_t* msg, size_t msg_len, size_t msg_stride,
                           const uint8_t* addrnd, uint8_t* sig);
/* SLH-DSA for the six SHA-2 parameter sets of FIPS 205 (section 11.2): slh_keygen_internal (Algorithm 18), slh_verify_internal (Algorithm 20) and
 * slh_sign_internal (Algorithm 19, below), batched, bytes in and bytes out.  HashSLH-DSA is not here.  The sets
 * have the SHAKE sets' (n, h, d, h', a, k, m) and sizes, and a `param` numbering of their own: PSF_SLHDSA_SHA2_* below, for these nine entry points only.
 * The hash functions, with the 22-byte compressed address ADRSc = layer 1 byte || tree 8 || type 1 || the last 12 bytes of ADRS:
 *   n = 16      F, PRF, H, T_l = Trunc_n(SHA-256(PK.seed || toByte(0, 64 - n) || ADRSc || M));
 *               H_msg = MGF1-SHA-256(R || PK.seed || SHA-256(R || PK.seed || PK.root || M), m)
 *   n = 24, 32  F, PRF as above; H, T_l = Trunc_n(SHA-512(PK.seed || toByte(0, 128 - n) || ADRSc || M));
 *               H_msg = MGF1-SHA-512(R || PK.seed || SHA-512(R || PK.seed || PK.root || M), m)
 *   PRF_msg     Trunc_n(HMAC-SHA-256(SK.prf, opt_rand || M)) at n = 16, Trunc_n(HMAC-SHA-512(SK.prf, opt_rand || M)) at n = 24, 32 (RFC 2104)
 * The block PK.seed || zeros is compressed once per lane at kernel entry; F, PRF and H are one compression past that midstate.
 * Argument lists, strides (pk_stride = 0: one key for all), PSF_SLHDSA_OP_*, the order of the PSF_ERR_PARAM checks, "nothing launched or written on
 * an error", count = 0, PSF_ERR_UNSUPPORTED above 2^31 - 1 instances and PSF_ERR_HIP without a device are exactly those of psf_slhdsa_sizes,
 * psf_slhdsa_workspace_bytes, psf_slhdsa_keygen(_dev) and psf_slhdsa_verify(_dev) above; so are the secrecy rules of keygen (WOTS+ secret values and
 * chain intermediates in registers only, every chain its 15 steps, no secret-dependent branch or address).
 * d_ws holds public values: keygen the chain ends (2^h' len n bytes per instance) | the leaves (2^h' n), each node as n / 4 big-endian 32-bit words,
 * and the last thing the call queues on `stream` sets every byte of d_ws to zero; verify the first 64 bytes of the MGF1 mask of H_msg (n > 16: the
 * inner SHA-512 digest passes through the same 64 bytes first) | the k FORS roots | the current node (32 bytes) | the len chain ends of the current
 * layer, and is NOT cleared.
 *   sign     psf_slhdsa_sha2_sign_workspace_bytes, psf_slhdsa_sha2_sign_dev and psf_slhdsa_sha2_sign have the argument lists and the semantics of
 *            psf_slhdsa_sign_workspace_bytes, psf_slhdsa_sign_dev and psf_slhdsa_sign above, with `param` a PSF_SLHDSA_SHA2_*: Algorithm 19 byte for
 *            byte; sk_stride = 0 means one key for all; d_addrnd NULL is the deterministic variant (opt_rand = PK.seed read from the key at the key's
 *            pitch), else n bytes per instance, contiguous; d_msg may be NULL when msg_len = 0; the order of the PSF_ERR_PARAM checks (msg_len must
 *            leave 3 n + msg_len a bit count that fits 64 bits); nothing launched or written on an error; count = 0 is PSF_OK after the param check;
 *            PSF_ERR_UNSUPPORTED above 2^31 - 1 instances; PSF_ERR_HIP without a device; the host form zeroes its device copies of sk and addrnd on
 *            every path out.  The workspace has the SHAKE twin's sections, order and sizes -- psf_slhdsa_sha2_sign_workspace_bytes(param, count)
 *            equals psf_slhdsa_sign_workspace_bytes of the set with the same (n, s / f) for every count -- each node as n / 4 big-endian 32-bit
 *            words; at n > 16 the public inner digest of H_msg passes through the instance's 64 digest bytes, as in verify; the last thing the call
 *            queues on `stream` sets every byte of d_ws to zero.  The two key blocks of HMAC and its inner digest are secret and exist in registers
 *            only; otherwise the secrecy rules are the twin's: the only stores of secret-derived values are R, the one revealed FORS secret value per
 *            tree and the WOTS+ value at its digit, and no branch, loop bound or address depends on a secret. */
enum { PSF_SLHDSA_SHA2_128S = 0, PSF_SLHDSA_SHA2_128F = 1, PSF_SLHDSA_SHA2_192S = 2, PSF_SLHDSA_SHA2_192F = 3, PSF_SLHDSA_SHA2_256S = 4,
       PSF_SLHDSA_SHA2_256F = 5 };
psf_status psf_slhdsa_sha2_sizes(int param, size_t* pk, size_t* sk, size_t* sig);
psf_status psf_slhdsa_sha2_workspace_bytes(int param, size_t count, int op, size_t* bytes);
psf_status psf_slhdsa_sha2_keygen_dev(int device, int param, size_t count, const uint8_t* d_sk_seed, const uint8_t* d_sk_prf, const uint8_t* d_pk_seed,
                                      uint8_t* d_pk, uint8_t* d_sk, void* d_ws, size_t ws_bytes, void* stream);
psf_status psf_slhdsa_sha2_verify_dev(int device, int param, size_t count, const uint8_t* d_pk, size_t pk_stride, const uint8_t* d_msg, size_t msg_len,
                                      size_t msg_stride, const uint8_t* d_sig, uint8_t* d_ok, void* d_ws, size_t ws_bytes, void* stream);
psf_status psf_slhdsa_sha2_keygen(int device, int param, size_t count, const uint8_t* sk_seed, const uint8_t* sk_prf, const uint8_t* pk_seed, uint8_t* pk,
                                  uint8_t* sk);
psf_status psf_slhdsa_sha2_verify(int device, int param, size_t count, const uint8_t* pk, size_t pk_stride, const uint8_t* msg, size_t msg_len, size_t msg_stride,
                                  const uint8_t* sig, uint8_t* ok);
psf_status psf_slhdsa_sha2_sign_workspace_bytes(int param, size_t count, size_t* bytes);
psf_status psf_slhdsa_sha2_sign_dev(int device, int param, size_t count, const uint8_t* d_sk, size_t sk_stride, const uint8_t* d_msg, size_t msg_len,
                                    size_t msg_stride, const uint8_t* d_addrnd, uint8_t* d_sig, void* d_ws, size_t ws_bytes, void* stream);
psf_status psf_slhdsa_sha2_sign(int device, int param, size_t count, const uint8_t* sk, size_t sk_stride, const uint8_t* msg, size_t msg_len, size_t msg_stride,
                                const uint8_t* addrnd, uint8_t* sig);
/* rot_minus_matrix (rotation_matrix.rs:85-96): mat[rows x cols] -> out[rows x rows*cols] */
psf_status psf_rot_minus_matrix(const int64_t* mat, size_t rows, size_t cols, int64_t* out);

/* ------------------------------------------------------------------------------------------------
 * PSFPerturbation (mp_perturbation.rs:57-62, impl PSF :193-403)
 *   A        = MatZq  n x m            -> uint64_t[n*m]
 *   Trapdoor = (R, sqrt(Sigma_2), (S, S~)) (mp_perturbation.rs:195)
 *                R            : int8_t[m_bar * n*k]           entries in {-1,0,1}
 *                sqrt(Sigma_2): double, lower triangular, packed by rows: row i holds i+1 entries,
 *                               m(m+1)/2 doubles (the Cholesky factor of :138)
 *                (S, S~)      : I_n (x) S_k and its GSO; a function of the parameters only, so it is
 *                               rebuilt inside the handle instead of being passed around
 *   Domain   = MatZ m x 1, Range = MatZq n x 1
 * ---------------------------------------------------------------------------------------------- */
typedef struct psfp_handle psfp_handle;

typedef struct {
  psf_gadget_params gp;
  double r;        /* rounding parameter (mp_perturbation.rs:60) */
  double s;        /* Gaussian parameter (mp_perturbation.rs:61) */
  int32_t device;  /* HIP device ordinal */
  uint32_t flags;  /* 0, or PSFP_FLAG_STRUCTURED_SQRT */
} psfp_params;

/* Opt-in: a STRUCTURED square root of Sigma_2 instead of the dense Cholesky factor of mp_perturbation.rs:138.  With Sigma = s^2 I,
 *   Sigma_2 = c [[alpha I - kappa R R^t, -kappa R], [-kappa R^t, beta I]],  c = r^2 / 2 pi, kappa = base^2 + 1, alpha = s^2 - 1, beta = alpha - kappa,
 * factors as B B^t with B = [[L_1, -g R], [0, h I]], L_1 = chol(c (alpha I - kappa (alpha / beta) R R^t)) (m_bar x m_bar), g = sqrt(c) kappa / sqrt(beta),
 * h = sqrt(c beta).  The perturbation is sampled as x_top = L_1 d_1 - g R d_2, x_bot = h d_2: a quarter of the FP64 work, a key of m_bar(m_bar+1)/2 doubles
 * instead of m(m+1)/2, trap_gen eight times cheaper.  Any square root of Sigma_2 gives the same distribution (the reference's sampler only needs
 * B B^t = Sigma_2); individual outputs differ from the dense path, so this is a different -- labelled -- algorithm, not the parity path.
 * d_2 is taken in fixed point (multiples of 2^-32) so that R d_2 is an exact integer sum.  In this mode the `sqrt_sigma2_packed` arguments of
 * psfp_load_key / psfp_export_key / psfp_export_sqrt_sigma2_rows hold L_1 (m_bar(m_bar+1)/2 doubles); psfp_load_key expects a factor produced with the
 * handle's (r, s). */
#define PSFP_FLAG_STRUCTURED_SQRT 2u

/* Limits: k <= 64, 1 < q < 2^62, and s * r * sqrt(m) < 2^23 (every coordinate of an in-domain vector then fits the three int8
 * digit planes of the Z_q products); PSF_ERR_UNSUPPORTED otherwise.  BASELINE's largest set (n=1024, q=2^60, s=1024, r=10)
 * reaches 3.6e6 of the 8.39e6 allowed. */
psf_status psfp_create(const psfp_params* params, psfp_handle** out);
void       psfp_destroy(psfp_handle*);
/* m = m_bar + n*k */
size_t     psfp_m(const psfp_handle*);

/* PSF::trap_gen (mp_perturbation.rs:221-244): samples A_bar, R on device, builds A = [A_bar | G - A_bar R]
 * (gadget_classical.rs:56-68), Sigma_2 and its Cholesky factor (mp_perturbation.rs:111-139).
 * PSF_ERR_NOT_PD if Sigma_2 is not positive definite (s too small). */
psf_status psfp_trap_gen(psfp_handle*, uint64_t seed);
/* PSFPerturbation::compute_sqrt_sigma_2 (mp_perturbation.rs:111-139) for Sigma = s_cov^2 * I using the
 * handle's R; replaces the handle's sqrt(Sigma_2) (the doctest at :89-107).  With PSFP_FLAG_STRUCTURED_SQRT only s_cov == s is
 * accepted (PSF_ERR_UNSUPPORTED otherwise): the structured factor's constants are rebuilt from s when a key is loaded. */
psf_status psfp_compute_sqrt_sigma_2(psfp_handle*, double s_cov);
/* The general form: `mat_sigma: &MatQ` of mp_perturbation.rs:111 is any symmetric m x m matrix (used as a full matrix at :125-126).
 * sigma_lower_packed: its lower triangle, row i holding i + 1 entries (m(m+1)/2 doubles).  PSF_ERR_NOT_PD if Sigma_2 is not positive
 * definite; PSF_ERR_UNSUPPORTED on a PSFP_FLAG_STRUCTURED_SQRT handle (that factor exists for Sigma = s^2 I only). */
psf_status psfp_compute_sqrt_sigma_2_dense(psfp_handle*, const double* sigma_lower_packed);
/* install / read back key material (host buffers).  Any of the out pointers may be NULL.
 * psfp_load_key(A, NULL, NULL): the PUBLIC key only -- what a verifier holds; f_a, check_domain and samp_d work (PSF::f_a takes `a` alone,
 *   mp_perturbation.rs:366), samp_p returns PSF_ERR_NO_KEY.
 * psfp_load_key(A, R, NULL): sqrt(Sigma_2) is recomputed from R with the handle's s, as trap_gen does (mp_perturbation.rs:227-231). */
psf_status psfp_load_key(psfp_handle*, const uint64_t* A, const int8_t* R, const double* sqrt_sigma2_packed);
/* (A, R) WITHOUT a factor and without computing one: the state PSFPerturbation::compute_sqrt_sigma_2 (mp_perturbation.rs:111-139, a pure function of
 * mat_r and mat_sigma) starts from.  A may be NULL (the handle's public matrix, if any, stays installed).  samp_p returns PSF_ERR_NO_KEY until
 * psfp_compute_sqrt_sigma_2 / _dense has produced the factor.  (psfp_load_key(A, R, NULL) instead runs the whole Cholesky with the handle's s.) */
psf_status psfp_load_trapdoor(psfp_handle*, const uint64_t* A, const int8_t* R);
psf_status psfp_export_key(const psfp_handle*, uint64_t* A, int8_t* R, double* sqrt_sigma2_packed);
/* rows [row0, row0 + nrows) of sqrt(Sigma_2) in the same packed form (row i holds i + 1 entries): the factor of BASELINE's
 * largest set is 60.5 GB, so a caller that inspects or ships it does so in row blocks */
psf_status psfp_export_sqrt_sigma2_rows(const psfp_handle*, size_t row0, size_t nrows, double* out);
/* the gadget part of the trapdoor tuple: S_k (k x k) and its Gram-Schmidt vectors (columns, k x k) */
psf_status psfp_export_gadget_basis(const psfp_handle*, int64_t* Sk, double* Sk_gso);

/* PSF::samp_d (mp_perturbation.rs:264-267): e[b] <- D_{Z^m, s*r} */
psf_status psfp_samp_d(psfp_handle*, uint64_t seed, uint64_t first_index, size_t B, int64_t* e);
/* PSF::samp_p (mp_perturbation.rs:304-336), B independent calls */
psf_status psfp_samp_p(psfp_handle*, uint64_t seed, uint64_t first_index, size_t B, const uint64_t* u, int64_t* e);
/* The same, asynchronous: returns once the work is enqueued (u has been staged and may be reused); e[] is complete when psfp_wait returns.  At most
 * two calls are in flight per handle (a third waits for the first).  The rows of call i cross PCIe (narrowed to int32 on the device, widened into e by
 * worker threads) while call i + 1 computes, so a loop of asynchronous calls runs at the device-resident rate; psfp_samp_p = psfp_samp_p_async +
 * psfp_wait.  psfp_wait returns the first non-OK status of the outstanding calls, oldest first (PSF_ERR_SAMPLER as psfp_samp_p would).
 * RULE: every other entry point that rewrites the key (psfp_trap_gen, psfp_load_key, psfp_load_trapdoor, psfp_compute_sqrt_sigma_2(_dense)) or uses the
 * handle's per-batch buffers (psfp_samp_p_dev, psfp_samp_d(_dev), psfp_f_a(_dev), psfp_samp_p_stages) first waits for the asynchronous calls in flight --
 * they never see a half-replaced key or share buffers with the new call -- and returns their status if one of them failed.  A handle is driven by one
 * thread at a time. */
psf_status psfp_samp_p_async(psfp_handle*, uint64_t seed, uint64_t first_index, size_t B, const uint64_t* u, int64_t* e);
psf_status psfp_wait(psfp_handle*);
/* Per-call status for a caller that keeps several batches (the shim's PendingBatch).  Every asynchronous call of a handle carries a ticket 0, 1, 2, ...:
 * psfp_async_next_ticket says which one the NEXT call will get; psfp_wait_ticket waits for that call (and the older one in flight, nothing newer) and returns ITS
 * status, however many other waits have joined it in the meantime (psfp_wait reports the first failure of everything outstanding and so consumes statuses of
 * calls the caller may not be asking about).  PSF_ERR_PARAM for a ticket never issued or older than the handle's last 8 joined calls.  (The synchronous
 * psfp_samp_p of a large batch is an asynchronous call + wait inside the library and takes a ticket too.) */
uint64_t   psfp_async_next_ticket(const psfp_handle*);
psf_status psfp_wait_ticket(psfp_handle*, uint64_t ticket);
/* PSF::f_a (mp_perturbation.rs:366-369): u[b] = A e[b] mod q; PSF_ERR_DOMAIN (u still written) if any
 * row fails check_domain */
psf_status psfp_f_a(psfp_handle*, size_t B, const int64_t* e, uint64_t* u);
/* PSF::check_domain (mp_perturbation.rs:396-402) for rows of length `len`; ok[b] = 0/1.  Decided as the reference decides it, in exact arithmetic:
 * ok[b] = (len == m and ||e_b||^2 <= s^2 m r^2) with s and r standing for the rationals those doubles denote (r = 1 for psfgpv_ / psfring_check_domain,
 * gpv.rs:219-224 and gpv_ring.rs:274-283).  The host forms floor(s^2 m r^2) in multi-limb integers from the mantissas and exponents of s and r, the kernel
 * sums the squares in 192 bits (no row of int64 wraps them, INT64_MIN included) and compares integers; nothing is rounded.  The same test is the d_ok of
 * X_f_a_dev and the PSF_ERR_DOMAIN of X_f_a. */
psf_status psfp_check_domain(psfp_handle*, size_t B, const int64_t* e, size_t len, uint8_t* ok);

/* One job over `count` handles, one per GPU of the node, each holding the same key (psfp_trap_gen with the same seed, or psfp_load_key):
 * the B rows are cut into contiguous shares (psf_shard_range), share i is computed by handles[i] on its own device, all devices at once.
 * Row b uses global index first_index + b, so the result equals psfp_samp_p on one handle bit for bit.  Host buffers (pageable is fine):
 * one worker thread per handle drives its device for the call (upload, samp_p, download), because HIP copies from / to pageable memory
 * block the issuing thread.  A handle may appear once in `handles`.  Every worker finishes and synchronises its stream before the call
 * returns, also after an error on another device; the first non-OK status in handle order is returned. */
psf_status psfp_samp_p_multi(psfp_handle* const* handles, int count, uint64_t seed, uint64_t first_index, size_t B, const uint64_t* u, int64_t* e);
/* this handle's window inside the last psfp_samp_p_multi call, in ms since that call began (host clock): its first samp_p launch
 * sequence enqueued / its last row landed in e; -1 if it had no rows.  Overlapping windows = the devices worked at the same time. */
psf_status psfp_get_multi_timing(const psfp_handle*, double* launched_ms, double* done_ms);

/* device-resident variants: d_u, d_e are HIP device pointers, stream is a hipStream_t (NULL = default).
 * Asynchronous with respect to the host; errors detected on device are reported by psfp_last_status. */
psf_status psfp_samp_p_dev(psfp_handle*, uint64_t seed, uint64_t first_index, size_t B,
                           const uint64_t* d_u, int64_t* d_e, void* stream);
/* count independent samp_p_dev calls in one submission.  Batch i: seeds[i], first_indices[i], targets d_u + i*B*n,
 * preimages d_e + i*B*m (m = psfp_m / psfgpv_m; for the ring type d = n(k+2)).  The bytes are those of
 *   for (i = 0; i < count; ++i) X_samp_p_dev(h, seeds[i], first_indices[i], B, d_u + i*B*n, d_e + i*B*m, stream);
 * Ordered on `stream` like samp_p_dev: it starts behind the work enqueued before it, and work enqueued after it sees every batch.
 * seeds / first_indices are host arrays; the call returns once everything is enqueued.  count == 0 or B == 0: PSF_OK, nothing enqueued.
 * Every check runs before anything is enqueued; asynchronous host-pointer calls in flight are drained first.  X_last_status afterwards: PSF_ERR_SAMPLER
 * if the sampler failed in ANY batch.  The nearest-plane types run batches that take one launch per 64-row block (C4) on two lanes (a second set
 * of per-batch buffers, allocated by the first such call with count >= 2, and two streams of the handle): one batch's solve, projection and
 * recombination overlap the other lane's walk.  Batches that fit the one-launch walk (C2) gain nothing from that and run in order on `stream`, as do
 * all batches with timing enabled (psfgpv_enable_timing; get_timing then describes the last batch).  psfp_samp_p_dev_many runs the batches in order
 * on `stream`. */
psf_status psfp_samp_p_dev_many(psfp_handle*, size_t count, const uint64_t* seeds, const uint64_t* first_indices, size_t B,
                                const uint64_t* d_u, int64_t* d_e, void* stream);
psf_status psfp_samp_d_dev(psfp_handle*, uint64_t seed, uint64_t first_index, size_t B, int64_t* d_e, void* stream);
psf_status psfp_f_a_dev(psfp_handle*, size_t B, const int64_t* d_e, uint64_t* d_u, uint8_t* d_ok, void* stream);
/* synchronises the stream of the last *_dev call and returns the device-side status of that call */
psf_status psfp_last_status(psfp_handle*);
/* synthetic uniform targets u <- Z_q^{B x n} (benches/psf.rs:35,60,87) written to device memory */
psf_status psfp_uniform_targets_dev(psfp_handle*, uint64_t seed, uint64_t first_index, size_t B, uint64_t* d_u, void* stream);
/* result rows for the inter-GPU gather: narrows count int64 preimage coordinates in device memory to
 * int32 (|e_i| <= 6 s r sqrt(m) for every parameter set of mp_perturbation.rs / gpv.rs); *d_overflow (device int) is
 * OR-ed with 1 if a value does not fit, so the caller can refuse to ship truncated rows */
psf_status psf_narrow_rows_dev(const int64_t* d_src, int32_t* d_dst, size_t count, int* d_overflow, int device, void* stream);

/* stage-level access for parity tests and profiling (host buffers; NULL = skip):
 * runs samp_p for B rows and copies out the intermediates of the reference's call stack
 *   d : B x m  standard normals fed to sqrt(Sigma_2)        (mp_perturbation.rs:315)
 *   x : B x m  centres  x = sqrt(Sigma_2) d
 *   p : B x m  perturbation p_i <- D_{Z,r,x_i}
 *   v : B x n  v = u - A p                                  (:318)
 *   z : B x nk gadget preimage                               (:321-326)
 */
psf_status psfp_samp_p_stages(psfp_handle*, uint64_t seed, uint64_t first_index, size_t B, const uint64_t* u,
                              double* d, double* x, int64_t* p, uint64_t* v, int64_t* z, int64_t* e);
/* per-kernel average duration (ms) of the last samp_p*_dev/samp_p call, measured with HIP events on the
 * launch stream when timing is enabled; names are ';'-separated in `names`. */
psf_status psfp_enable_timing(psfp_handle*, int on);
psf_status psfp_get_timing(psfp_handle*, char* names, size_t names_len, double* ms, size_t* count);
/* which forms a samp_p pass takes (diagnostic, read-only).  One pass over B preimages picks a product form, a normals layout, a rounding kernel, a Z_q
 * form, a gadget walk and a recombination from B, the key's shape and the buffers the handle holds; every form gives the same rows.
 *   psfp_query_plan    : the plan a pass over B preimages would take on the handle as it stands -- nothing is launched, allocated or changed
 *                        (what the call would derive from B for its buffers is computed for the query)
 *   psfp_get_last_plan : the plan of the last pass that ran (PSF_ERR_NO_KEY before the first).  A device-pointer call is one pass; a host-pointer call
 *                        of 2^20 coordinates or more runs in slices, each a pass of its own.
 * Both fill fields[0 .. PSFP_PLAN_FIELDS) in the order of the PSFP_PLAN_* indices; count is the room in `fields`. */
enum {
  PSFP_PLAN_ONE_LAUNCH = 0,   /* 1: the whole call in one launch (small keys, up to 64 preimages); the other fields are then the defaults */
  PSFP_PLAN_PRODUCT,          /* x = sqrt(Sigma_2) d: PSFP_PRODUCT_* */
  PSFP_PLAN_RT, PSFP_PLAN_NB, PSFP_PLAN_NCG,   /* 16-row tiles x fragments of 16 preimages per wave; column groups of 16 NB preimages */
  PSFP_PLAN_BC,               /* dense normals stream of bc = 1 ... 16 preimages (0: fragments or chunks) */
  PSFP_PLAN_COMPACT,          /* 1: compact normals stream, 0: chunk stream */
  PSFP_PLAN_GR, PSFP_PLAN_GC, /* PSFP_PRODUCT_BIG: super-tile of 8 x 4 or 16 x 2 workgroups */
  PSFP_PLAN_TAIL,             /* 1: rounding and syndrome in one launch behind the product (one or two preimages, compact key copies present) */
  PSFP_PLAN_ROUND,            /* PSFP_ROUND_* */
  PSFP_PLAN_SYN_FORM,         /* v = u - A p: PSFP_ZQ_* */
  PSFP_PLAN_SYN_SPLITS, PSFP_PLAN_SYN_FOLD128, PSFP_PLAN_SYN_POW2, PSFP_PLAN_SYN_WAVE_COMBINE,
  PSFP_PLAN_GADGET,           /* PSFP_GADGET_* */
  PSFP_PLAN_K32,              /* gadget kernels: the k <= 32 instantiation */
  PSFP_PLAN_GQ_P,             /* PSFP_GADGET_QUEUE: problems per wave */
  PSFP_PLAN_RECOMBINE,        /* e = p + [R; I] z: PSFP_RECOMBINE_* */
  PSFP_PLAN_NBF,              /* PSFP_RECOMBINE_WG: fragments of 16 preimages per column group */
  PSFP_PLAN_RC_BIG,           /* PSFP_RECOMBINE_TILES: the 256 x 256 tiles first */
  PSFP_PLAN_RSPLITS,          /* PSFP_RECOMBINE_TILES: K splits of the 128 x 128 kernel */
  PSFP_PLAN_FIELDS
};
enum { PSFP_PRODUCT_TASKS = 0, PSFP_PRODUCT_TILES64 = 1, PSFP_PRODUCT_TILES32 = 2, PSFP_PRODUCT_TILES96 = 3, PSFP_PRODUCT_BIG = 4 };
enum { PSFP_ROUND_TAB = 0, PSFP_ROUND_TAB_ROW = 1, PSFP_ROUND_LEAN = 2, PSFP_ROUND_WAVE = 3 };
enum { PSFP_ZQ_SMALL = 0, PSFP_ZQ_SMALL32 = 1, PSFP_ZQ_MFMA = 2 };
enum { PSFP_GADGET_WAVE = 0, PSFP_GADGET_ROW = 1, PSFP_GADGET_QUAD = 2, PSFP_GADGET_QUEUE = 3, PSFP_GADGET_LOCKSTEP = 4 };
enum { PSFP_RECOMBINE_SMALL = 0, PSFP_RECOMBINE_SMALL2 = 1, PSFP_RECOMBINE_WG = 2, PSFP_RECOMBINE_TILES = 3 };
psf_status psfp_query_plan(const psfp_handle*, size_t B, int* fields, size_t count);
psf_status psfp_get_last_plan(const psfp_handle*, int* fields, size_t count);

/* ------------------------------------------------------------------------------------------------
 * PSFGPV (gpv.rs:53-57, impl PSF :59-225)
 *   A        = MatZq n x m
 *   Trapdoor = (short_base, short_base_gso) (gpv.rs:61): both m x m.  They cross this ABI TRANSPOSED: row i of
 *              `basis_t` / `gso_t` is basis vector i, i.e. column i of the reference's MatZ / MatQ
 *              (gen_short_basis_for_trapdoor, short_basis_classical.rs:54-63; MatQ::gso, gpv.rs:91).
 *   samp_p (gpv.rs:152-161): sol = A.solve_gaussian_elimination(u); e = sol + SampleD(basis, gso, -sol, s), SampleD in the
 *   batched blocked form of tools_amd/csrc/psf_np_kernels.hpp (any lattice dimension that fits the device memory).
 *   The elimination is factored once per key (pivot columns + n x n operator); it returns the same particular
 *   solution as eliminating [A | u] per call with unit pivots and free variables 0.
 *   Precision of the centres.  The reference holds the centre in exact rationals (MatQ, gpv.rs:158-160); the walk here keeps its running
 *   projections in doubles.  With the centre -sol (entries up to q on n coordinates) the error of a centre, in units of that draw's width
 *   s / |b~_i|, is about 2^-53 q sqrt(n) / s whatever the basis.  Keys with q sqrt(n) <= 2^13 s (C2, C4: 2^-47) are sampled in one pass at
 *   a relative centre error <= 2^-40; for larger moduli -- every q < 2^62 -- samp_p runs TWO passes: the first finds a short element e1 of
 *   the coset A e = u, the second samples e1 + D_{Lambda, s, -e1}, whose centres are of ordinary size (|e1| ~ s sqrt(m)): the output
 *   distribution is that of gpv.rs:160 for any e1 (GPV08), so the first pass's imprecision cannot reach it, and the relative centre error
 *   of the pass that matters is <= 2^-35 (asserted against 100-digit arithmetic in tests/test_oracle_centre_precision.py; the floor is
 *   the double-precision Gram-Schmidt data, 1e-13 relative).  psfgpv_two_pass() says which form a handle uses.
 * ---------------------------------------------------------------------------------------------- */
typedef struct psfgpv_handle psfgpv_handle;
typedef struct {
  psf_gadget_params gp;
  double s;        /* Gaussian parameter (gpv.rs:56) */
  int32_t device;
  uint32_t flags;  /* reserved, 0 */
} psfgpv_params;

psf_status psfgpv_create(const psfgpv_params* params, psfgpv_handle** out);
void       psfgpv_destroy(psfgpv_handle*);
size_t     psfgpv_m(const psfgpv_handle*);
/* PSF::trap_gen (gpv.rs:83-94): A, R as for PSFPerturbation; short basis and its GSO built on device.
 * PSF_ERR_NO_SOLUTION if A has fewer than n unit pivots mod q. */
psf_status psfgpv_trap_gen(psfgpv_handle*, uint64_t seed);
psf_status psfgpv_load_key(psfgpv_handle*, const uint64_t* A, const int32_t* basis_t, const double* gso_t);
psf_status psfgpv_export_key(const psfgpv_handle*, uint64_t* A, int8_t* R, int32_t* basis_t, double* gso_t);
psf_status psfgpv_samp_d(psfgpv_handle*, uint64_t seed, uint64_t first_index, size_t B, int64_t* e);         /* gpv.rs:113-116 */
psf_status psfgpv_samp_p(psfgpv_handle*, uint64_t seed, uint64_t first_index, size_t B, const uint64_t* u, int64_t* e);
psf_status psfgpv_samp_p_dev(psfgpv_handle*, uint64_t seed, uint64_t first_index, size_t B, const uint64_t* d_u, int64_t* d_e, void* stream);
/* as psfp_samp_p_dev_many; psfgpv_get_nearest_plane_form reports the form shared by the batches, its reruns count covers every batch */
psf_status psfgpv_samp_p_dev_many(psfgpv_handle*, size_t count, const uint64_t* seeds, const uint64_t* first_indices, size_t B,
                                  const uint64_t* d_u, int64_t* d_e, void* stream);
/* gpv.rs:152-161 on host buffers without waiting (the transport of psfp_samp_p_async: rows narrowed to int32 on the device, chunk transfers by the DMA engines into
 * per-call pinned rings, widened into e by worker threads): returns once the work is enqueued (u may be reused), e[] is complete when psfgpv_wait returns.  At most two
 * calls in flight per handle; the rows of call i cross PCIe while call i + 1 walks.  psfgpv_wait returns the first non-OK status of the outstanding calls, oldest first:
 * PSF_ERR_SAMPLER as psfgpv_samp_p would; PSF_ERR_UNSUPPORTED if a row entry did not fit 32 bits (the synchronous call copies 64-bit rows in that case). */
psf_status psfgpv_samp_p_async(psfgpv_handle*, uint64_t seed, uint64_t first_index, size_t B, const uint64_t* u, int64_t* e);
psf_status psfgpv_wait(psfgpv_handle*);
uint64_t   psfgpv_async_next_ticket(const psfgpv_handle*);                    /* as psfp_async_next_ticket / psfp_wait_ticket */
psf_status psfgpv_wait_ticket(psfgpv_handle*, uint64_t ticket);
psf_status psfgpv_f_a(psfgpv_handle*, size_t B, const int64_t* e, uint64_t* u);                               /* gpv.rs:190-193 */
psf_status psfgpv_f_a_dev(psfgpv_handle*, size_t B, const int64_t* d_e, uint64_t* d_u, uint8_t* d_ok, void* stream);
psf_status psfgpv_check_domain(psfgpv_handle*, size_t B, const int64_t* e, size_t len, uint8_t* ok);         /* gpv.rs:219-224 */
psf_status psfgpv_uniform_targets_dev(psfgpv_handle*, uint64_t seed, uint64_t first_index, size_t B, uint64_t* d_u, void* stream);
psf_status psfgpv_last_status(psfgpv_handle*);
/* HIP-event durations (ms) of the last samp_p call (0 if timing was off): the solve kernel, and the whole nearest plane
 * (initial projection, per block one sampling and one update launch, recombination) */
psf_status psfgpv_enable_timing(psfgpv_handle*, int on);
psf_status psfgpv_get_timing(psfgpv_handle*, double* solve_ms, double* nearest_plane_ms);
/* diagnostic of the last samp_p call: the number of 64-row blocks the nearest-plane walk (gpv.rs:160) was cut into, and whether
 * e = sum z_i b_i was recombined by the 64-bit integer kernel (1) instead of the int8 matrix-core planes (0) -- the former when a
 * basis entry or a drawn z_i does not fit two balanced base-256 digits (|.| > 32639); the result is the same either way */
psf_status psfgpv_get_nearest_plane_stats(psfgpv_handle*, size_t* blocks, size_t* generic_recombination);
/* The walk of gpv.rs:160 has two launch forms with identical results: ONE launch (k_np_walk<G>: sampler workgroups and updater workgroups that hand blocks to each
 * other through device memory; chosen when the device's occupancy figures say every workgroup is resident at once) and one launch per 64-row block (k_np_step<G>).
 * A large batch of the second form walks as two column ranges side by side on two streams of the handle (the matrix-core update tiles of one range run beside the
 * samplers of the other), joined on the caller's stream before the call's last kernel: form 2.
 * form: 1 / 0 / 2 as launched by the last call; preimages_per_wave: G; reruns: walks of this handle since its creation in which a workgroup of the one-launch form gave
 * up waiting for another (a GPU shared with other work) and the call was walked again, inside the same call, by a form without waits between workgroups
 * (k_np_walk_solo).  Contention costs time, never the call: PSF_ERR_SAMPLER is reserved for SampleZ itself.  One-launch walks of one process take turns per device. */
psf_status psfgpv_get_nearest_plane_form(psfgpv_handle*, int* form, int* preimages_per_wave, size_t* blocks, uint64_t* reruns);
/* 1 if samp_p of this handle draws in two passes (large moduli, see "Precision of the centres" above), else 0 */
int psfgpv_two_pass(const psfgpv_handle*);

/* ------------------------------------------------------------------------------------------------
 * PSFGPVRing (gpv_ring.rs:62-67, impl PSF :69-284) over R_q = Z_q[X]/(X^n + 1)
 *   A        = MatPolynomialRingZq 1 x (k+2)  -> uint64_t[(k+2) * n], polynomial j at a + j*n, constant term first
 *   Trapdoor = (r, e), two 1 x k MatPolyOverZ  -> int64_t[k * n] each (gadget_ring.rs:62-81)
 *   Domain   = MatPolyOverZ (k+2) x 1          -> int64_t[(k+2) * n] per call
 *   Range    = one element of R_q               -> uint64_t[n] per call
 * Any modulus 1 < q < 2^62 (GadgetParametersRing carries an arbitrary ModulusPolynomialRingZq, gadget_parameters.rs:73-81): R_q products by the NTT
 * kernel where q allows and by the exact schoolbook kernel elsewhere, the walk in two passes where q sqrt(n) > 2^13 s (see PSFGPV above).
 * samp_p (gpv_ring.rs:160-212) works on the coefficient embedding: the short basis
 * (gen_short_basis_for_trapdoor_ring, short_basis_ring.rs:64-79), rot^-(iota(a)) (rotation_matrix.rs:85-96), the
 * elimination and the Gram-Schmidt vectors are built ONCE per key here, where the reference rebuilds them per call.
 * f_a (gpv_ring.rs:243-247) is the R_q product a * sigma, evaluated as rot^-(iota(a)) iota(sigma) on the int8 matrix cores.
 * ---------------------------------------------------------------------------------------------- */
typedef struct psfring_handle psfring_handle;
typedef struct {
  psf_gadget_params gp;   /* from psf_gadget_params_ring_default: m_bar = k + 2 */
  double s;               /* gpv_ring.rs:65 */
  double s_td;            /* gpv_ring.rs:66 */
  int32_t device;
  uint32_t flags;
} psfring_params;

psf_status psfring_create(const psfring_params* params, psfring_handle** out);
void       psfring_destroy(psfring_handle*);
/* PSF::trap_gen (gpv_ring.rs:91-98) */
psf_status psfring_trap_gen(psfring_handle*, uint64_t seed);
psf_status psfring_load_key(psfring_handle*, const uint64_t* a, const int64_t* r, const int64_t* e);
/* a, r, e as above; basis_t / gso_t: d x d with d = n(k+2), row c = embedded basis vector c (any may be NULL) */
psf_status psfring_export_key(const psfring_handle*, uint64_t* a, int64_t* r, int64_t* e, int32_t* basis_t, double* gso_t);
psf_status psfring_samp_d(psfring_handle*, uint64_t seed, uint64_t first_index, size_t B, int64_t* sigma);            /* :118-122 */
psf_status psfring_samp_p(psfring_handle*, uint64_t seed, uint64_t first_index, size_t B, const uint64_t* u, int64_t* sigma);
psf_status psfring_samp_p_dev(psfring_handle*, uint64_t seed, uint64_t first_index, size_t B, const uint64_t* d_u, int64_t* d_sigma, void* stream);
/* as psfgpv_samp_p_dev_many */
psf_status psfring_samp_p_dev_many(psfring_handle*, size_t count, const uint64_t* seeds, const uint64_t* first_indices, size_t B,
                                   const uint64_t* d_u, int64_t* d_sigma, void* stream);
/* gpv_ring.rs:160-212 without waiting: as psfgpv_samp_p_async / psfgpv_wait */
psf_status psfring_samp_p_async(psfring_handle*, uint64_t seed, uint64_t first_index, size_t B, const uint64_t* u, int64_t* sigma);
psf_status psfring_wait(psfring_handle*);
uint64_t   psfring_async_next_ticket(const psfring_handle*);
psf_status psfring_wait_ticket(psfring_handle*, uint64_t ticket);
psf_status psfring_f_a(psfring_handle*, size_t B, const int64_t* sigma, uint64_t* u);                                  /* :243-247 */
psf_status psfring_f_a_dev(psfring_handle*, size_t B, const int64_t* d_sigma, uint64_t* d_u, uint8_t* d_ok, void* stream);
psf_status psfring_check_domain(psfring_handle*, size_t B, const int64_t* sigma, size_t len, uint8_t* ok);            /* :274-283 */
psf_status psfring_uniform_targets_dev(psfring_handle*, uint64_t seed, uint64_t first_index, size_t B, uint64_t* d_u, void* stream);
psf_status psfring_last_status(psfring_handle*);
psf_status psfring_enable_timing(psfring_handle*, int on);
psf_status psfring_get_timing(psfring_handle*, double* solve_ms, double* nearest_plane_ms);
psf_status psfring_get_nearest_plane_form(psfring_handle*, int* form, int* preimages_per_wave, size_t* blocks, uint64_t* reruns);

#ifdef __cplusplus
}
#endif
#endif
