/*
 * mvk.h — C ABI of libmvk.so: hand-written HIP (gfx950 / CDNA4) kernels for the multimodal-VAE
 * training hot path (MMVAE / MoPoE / MVTCAE forward + ELBO + backward + Adam).
 *
 * The reference (AgatheSenellart/MultiVae) has no FFI: its "operator API" is Python.
 * Each entry point below therefore names the reference Python function(s) it replaces (file:line,
 * relative to /root/reference/src/multivae).  Host code (multivae_amd/, Python on PyTorch-ROCm) binds
 * these through ctypes; INTEGRATION.md shows the binding a MultiVae maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous fp32 unless stated otherwise; the caller owns all
 *     memory; the library never allocates, frees, retains a pointer past the call, or synchronises;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it; calls are re-entrant per stream;
 *   - return value: 0 = MVK_OK, <0 = error (MVK_EINVAL bad argument, MVK_ELAUNCH launch failure);
 *   - noise is always an input buffer: results never depend on an RNG stream;
 *   - gradient outputs documented "+=" are ACCUMULATED into the caller's buffer: zero it first if needed.  Every
 *     reduction is deterministic: split-K slices, column-sum partials and per-workgroup weight-gradient slabs are
 *     written to caller-owned scratch and added in a fixed order (an entry point that is given no scratch falls back
 *     to fp32 atomicAdd, the only non-reproducible path);
 *   - there is no hidden global state, with TWO documented exceptions, both explicit begin / end pairs that the host
 *     owns and that are per device: (1) mvk_defer_begin / mvk_defer_flush / mvk_defer_end — between begin and end the
 *     ordered finishes of leaf gradients that target the registered flat gradient buffer are queued in a caller-owned
 *     arena and run as one launch at flush; (2) mvk_prof_enable / mvk_prof_disable — device-timestamp records of
 *     the launches in between are written to a caller-owned buffer.  Neither survives its end call; with neither
 *     active every entry point is a pure function of its arguments.
 */
#ifndef MVK_H
#define MVK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVK_OK 0
#define MVK_EINVAL (-1)
#define MVK_ELAUNCH (-2)

#define MVK_MAX_MODALITIES 8
#define MVK_MVAE_MAX_SUBSETS 32  /* subsets of one MVAE objective (joint + unimodal + k random ones) */
#define MVK_IWAE_MAX_EXPERTS 32 /* experts of the mixture posterior in mvk_iwae_logw (MoPoE: 2^5 - 1 subsets) */

/* decoder output distributions — models/base/base_utils.py:62-87 (set_decoder_dist) */
#define MVK_DIST_NORMAL 0
#define MVK_DIST_LAPLACE 1
#define MVK_DIST_BERNOULLI 2
#define MVK_DIST_CATEGORICAL 3 /* x * log_softmax(recon + 1e-6) over the last dimension (base_utils.py:28-57) */

/* activations fused into GEMM/conv epilogues */
#define MVK_ACT_NONE 0
#define MVK_ACT_RELU 1
#define MVK_ACT_SIGMOID 2
#define MVK_ACT_LEAKY02 3 /* LeakyReLU(0.2) (models/nn/mmnist.py:222-246, cub.py:250-293) */

/* latent families of MMVAE — models/mmvae/mmvae_model.py:44-49,66-74 */
#define MVK_FAMILY_NORMAL 0
#define MVK_FAMILY_LAPLACE_SOFTMAX 1
#define MVK_FAMILY_NORMAL_SOFTPLUS 2 /* std kernels only (MMVAE+): std = softplus(lv) + 1e-6, density = Normal */

int mvk_version(void);

/* ------------------------------------------------------------------------------------------------
 * Fused posterior aggregation + reparameterisation + Gaussian KL
 * ------------------------------------------------------------------------------------------------ */

/* MoPoE: per-subset PoE (+N(0,I) expert on the full subset), subset selection, z = mu + exp(lv/2) eps,
 * all-subset weighted KL.  Replaces models/base/base_utils.py:122-130 (poe), :150-172
 * (rsample_from_gaussian), models/mopoe/mopoe_model.py:274-350 (inference), :249-262 (_poe_fusion),
 * :435-465 / :417-433 (mixture component selection, given as `sel`), :108-145 (calc_joint_divergence).
 *   mu, lv        HOST arrays of M device pointers, each [B,L], modalities in PoE summation order
 *                 (the reference stacks a subset's experts in sorted-name order, mopoe_model.py:88-101)
 *   subset_masks  device int32 [S]: bit i set = modality i (position in mu/lv) belongs to the subset;
 *                 subsets in the reference's enumeration order (mopoe_model.py:71-80)
 *   sel           device int32 [B]: subset index whose posterior row b samples from
 *   weights       device [S,B] or NULL (= 1/S)
 *   eps           device [K,B,L]
 * outputs
 *   z [K,B,L]; kld_rows [B] = sum_s w[s,b] KL_s[b]; mus_out, lvs_out [S,B,L] (both or neither);
 *   joint_mu, joint_lv [B,L] (both or neither)
 */
int mvk_mopoe_posterior_fwd(const float* const* mu, const float* const* lv, int M, const int32_t* subset_masks,
                            int S, const int32_t* sel, const float* weights, const float* eps, int K, int B,
                            int L, float* z, float* kld_rows, float* mus_out, float* lvs_out, float* joint_mu,
                            float* joint_lv, void* stream);

/* backward of the above.  dz [K,B,L]; gkld_rows [B] = upstream gradient of kld_rows (NULL = 0).
 * dmu, dlv: HOST arrays of M device pointers [B,L], overwritten. */
int mvk_mopoe_posterior_bwd(const float* const* mu, const float* const* lv, int M, const int32_t* subset_masks,
                            int S, const int32_t* sel, const float* weights, const float* eps, const float* dz,
                            int K, int B, int L, const float* gkld_rows, float* const* dmu, float* const* dlv,
                            void* stream);

/* MVTCAE: PoE over all modalities (no prior expert, eps 1e-8), joint KL and per-modality conditional
 * KLs.  Replaces models/mvtcae/mvtcae_model.py:110-169 (_modality_encode masks, _inference) and the KL
 * arithmetic of :42-108.  masks: HOST array of M device uint8 [B] pointers (entries may be NULL), or NULL.
 * outputs: z [K,B,L]; joint_kl_rows [B]; cond_kl_rows [M,B]; joint_mu, joint_lv [B,L] (both or neither). */
int mvk_mvtcae_posterior_fwd(const float* const* mu, const float* const* lv, const uint8_t* const* masks,
                             int M, const float* eps, int K, int B, int L, float* z, float* joint_kl_rows,
                             float* cond_kl_rows, float* joint_mu, float* joint_lv, void* stream);

/* backward: gjoint_rows [B], gcond_rows [M,B] = upstream gradients of the two KL outputs (NULL = 0). */
int mvk_mvtcae_posterior_bwd(const float* const* mu, const float* const* lv, const uint8_t* const* masks,
                             int M, const float* eps, const float* dz, int K, int B, int L,
                             const float* gjoint_rows, const float* gcond_rows, float* const* dmu,
                             float* const* dlv, void* stream);

/* Diagonal Gaussian q = N(mu, exp(lv)): w[k,b,:] = mu[b,:] + exp(lv[b,:] / 2) eps[k,b,:] and kl_rows[b] =
 * -1/2 sum_l (1 - exp(lv) - mu^2 + lv) = KL(q || N(0,I)): the modality-specific ("style") latents of MoPoE
 * (mopoe_model.py:171-178 rsample, :212-221 style_kld).  mu, lv [B,L]; eps, w [K,B,L].  bwd: dw [K,B,L] (nullable),
 * gkl [B] (nullable) -> dmu, dlv [B,L] (overwritten). */
int mvk_gauss_sample_kl_fwd(const float* mu, const float* lv, const float* eps, int K, int B, int L, float* w,
                            float* kl_rows, void* stream);
int mvk_gauss_sample_kl_bwd(const float* mu, const float* lv, const float* eps, const float* dw, const float* gkl,
                            int K, int B, int L, float* dmu, float* dlv, void* stream);

/* Conditional latent (CVAE, cvae_model.py:145-172): the K samples of q = N(mu, exp(lv)), the conditioning data and the KL to a
 * learned prior in ONE launch, written as the decoder's input.  mu, lv [B,L]; pmu, plv [B,L], both given or both NULL (NULL = the
 * N(0,I) prior; the NULL form and two arrays of zeros write the same bits); eps [K,B,L]; cond: HOST array of n_cond device
 * pointers, piece j is [B, cond_dims[j]] (cond_dims: HOST array, every entry >= 1), 0 <= n_cond <= MVK_MAX_MODALITIES,
 * C = sum_j cond_dims[j].  Outputs: zc [K,B,L+C], every entry written once:
 *   zc[k,b,:L] = mu[b] + exp(lv[b] / 2) eps[k,b];   zc[k,b,L+off_j : L+off_j+C_j] = cond[j][b] for every k (bit-exact copies);
 * kl_rows [B] (nullable: generating from the prior needs the sample only) =
 *   1/2 sum_l (plv - lv + exp(lv - plv) + (mu - pmu)^2 exp(-plv) - 1)     (base_utils.py:111-119).
 * L + C may be odd (rows of zc are then not 16-byte aligned: the copy is scalar); the copy of the conditioning columns is spread
 * over workgroups of its own.  No atomics, bit-reproducible, B = 0 is MVK_OK and writes nothing.
 * bwd: dzc [K,B,L+C] (nullable; only the first L columns of each row are read, at row stride L + C: the conditioning data gets
 * no gradient), gkl [B] (nullable) -> dmu, dlv [B,L] and dpmu, dplv [B,L] (NULL exactly when pmu is NULL), all OVERWRITTEN,
 * everything recomputed from the inputs:
 *   dmu = sum_k dz + gkl (mu - pmu) exp(-plv);        dlv  = 1/2 exp(lv/2) sum_k dz eps + gkl 1/2 (exp(lv - plv) - 1);
 *   dpmu = -gkl (mu - pmu) exp(-plv);                 dplv = gkl 1/2 (1 - exp(lv - plv) - (mu - pmu)^2 exp(-plv)). */
int mvk_cond_latent_fwd(const float* mu, const float* lv, const float* pmu, const float* plv, const float* eps,
                        const float* const* cond, const int* cond_dims, int n_cond, int K, int B, int L, float* zc,
                        float* kl_rows, void* stream);
int mvk_cond_latent_bwd(const float* mu, const float* lv, const float* pmu, const float* plv, const float* eps,
                        const float* dzc, const float* gkl, int K, int B, int L, int C, float* dmu, float* dlv,
                        float* dpmu, float* dplv, void* stream);

/* MHVAE level (models/mhvae/mhvae_model.py:119-184 subset_encode, base_utils.py:122-130 poe, :111-119 kl_divergence): for every
 * subset s < S of the modalities, row b and element f, the product of the subset's available experts and the prior, one sample
 * and the KL to the prior, in ONE launch for all subsets of a level of the hierarchy.  Experts j of (s, b): the e < E with bit e of
 * member[s] set and masks[e][b] != 0, and the prior (always):
 *   T_j = 1 / (exp(lv_j) + 1e-8);   P = sum_j T_j;   jmu = sum_j mu_j T_j / P;   jlv = log(1 / P);
 *   z[s,b,f] = jmu + exp(jlv / 2) eps[s,b,f]   (eps NULL: z = jmu, the reference's return_mean);
 *   kl_rows[s,b] = sum_f 1/2 (plv - jlv + exp(jlv - plv) + (jmu - pmu)^2 / exp(plv) - 1)   (no 1e-8 in the KL).
 * A masked-out expert has T = 0 (the reference's log-variance of +inf, :88-101): nothing of it is read and its gradients are zeros.
 * mu, lv: HOST arrays of E device pointers, 1 <= E <= MVK_MAX_MODALITIES; masks: HOST array of E device uint8 [B] pointers
 * (entries may be NULL = all available) or NULL; member: HOST array of S bitmasks, 1 <= S <= MVK_MHVAE_MAX_SUBSETS, each non-zero
 * and below 2^E, every expert in at least one.  The host tables are copied into the launch: the call is capturable.  Two layouts,
 * anything else is MVK_EINVAL:
 *   shared = 1  every mu[e], lv[e] is [B,F] and serves each subset that holds e; pmu = plv = NULL: the prior is N(0, I), an expert
 *               with T = 1 / (1 + 1e-8) (the deepest level, :126-143);
 *   shared = 0  mu[e], lv[e] are [S_e,B,F], one block per subset holding e, in increasing subset order; pmu, plv [S,B,F], both
 *               required (the lower levels, :150-184, where every posterior depends on the subset's own z).
 * eps, z [S,B,F]; kl_rows [S,B]; F = the flattened per-row size of the level's latent, S B (F + 1) < 2^38.  16-byte accesses when F % 4 == 0 and every
 * pointer is 16-byte aligned, scalar ones otherwise.  No atomics: the row sums are taken in a fixed order, the result is
 * bit-reproducible.  B = 0 is MVK_OK and writes nothing.
 * bwd: dz [S,B,F] (nullable), gkl [S,B] (nullable) -> dmu[e], dlv[e] (HOST arrays of E device pointers, the shapes of mu[e], lv[e]),
 * dpmu, dplv [S,B,F] (NULL exactly when pmu is NULL), all OVERWRITTEN, everything recomputed from the forward's inputs.  With
 * a_j = T_j / P, vp = exp(plv):
 *   G_mu = dz + gkl (jmu - pmu) / vp;          G_P = -1/2 dz eps P^(-3/2) + 1/2 gkl (1 / P - 1 / (P^2 vp));
 *   dT_j = G_mu (mu_j - jmu) / P + G_P;        dmu_j = G_mu a_j;        dlv_j = -dT_j exp(lv_j) T_j^2;
 *   dpmu = (as an expert) - gkl (jmu - pmu) / vp;      dplv = (as an expert) + 1/2 gkl (1 - 1 / (P vp) - (jmu - pmu)^2 / vp).
 * shared = 1: the gradient of expert e at (b, f) is the sum over the subsets holding e, taken in increasing s in registers. */
#define MVK_MHVAE_MAX_SUBSETS 255 /* subsets of one mvk_mhvae_level_* call (2^8 - 1: every non-empty subset of 8 modalities) */
int mvk_mhvae_level_fwd(const float* const* mu, const float* const* lv, const uint8_t* const* masks, int E,
                        const int32_t* member, int S, int shared, const float* pmu, const float* plv, const float* eps, int B,
                        int F, float* z, float* kl_rows, void* stream);
int mvk_mhvae_level_bwd(const float* const* mu, const float* const* lv, const uint8_t* const* masks, int E,
                        const int32_t* member, int S, int shared, const float* pmu, const float* plv, const float* eps,
                        const float* dz, const float* gkl, int B, int F, float* const* dmu, float* const* dlv, float* dpmu,
                        float* dplv, void* stream);

/* TELBO stage two (models/telbo/telbo_model.py:101-124): the samples of all M unimodal posteriors and the reference's row "KL",
 * which takes the JOINT encoder's log-variance in the place of the modality's own, in ONE launch for all modalities:
 *   z[m,b,l]      = mu_m[b,l] + exp(lv_m[b,l] / 2) eps[m,b,l];
 *   kld_rows[m,b] = -1/2 sum_l (1 + joint_lv[b,l] - mu_m[b,l]^2 - exp(lv_m[b,l])).
 * joint_lv [B,L]; mu, lv: HOST arrays of M device pointers ([B,L] each), 1 <= M <= MVK_MAX_MODALITIES, copied into the launch (the
 * call is capturable); eps, z [M,B,L]; kld_rows [M,B].  Any L >= 1.  No atomics: a row sum is taken in a fixed order, the result
 * is bit-reproducible.  B = 0 is MVK_OK and writes nothing; a bad argument is MVK_EINVAL before any launch.
 * bwd: dz [M,B,L] (nullable), gkld [M,B] (nullable) -> dmu[m], dlv[m] [B,L] (HOST arrays of M device pointers) and djoint_lv [B,L]
 * (nullable: not wanted), all OVERWRITTEN, everything recomputed from the forward's inputs:
 *   dmu_m = dz_m + gkld[m,b] mu_m;     dlv_m = 1/2 exp(lv_m / 2) eps_m dz_m + 1/2 gkld[m,b] exp(lv_m);
 *   djoint_lv[b,l] = -1/2 sum_m gkld[m,b]   (added in increasing m). */
int mvk_telbo_latent_fwd(const float* joint_lv, const float* const* mu, const float* const* lv, int M, const float* eps,
                         int B, int L, float* z, float* kld_rows, void* stream);
int mvk_telbo_latent_bwd(const float* const* mu, const float* const* lv, int M, const float* eps, const float* dz,
                         const float* gkld, int B, int L, float* const* dmu, float* const* dlv, float* djoint_lv,
                         void* stream);

/* Masked autoregressive flows (MAF, models/nn/flows.py; JNF: models/jnf/jnf_model.py:165-183 `_compute_ljm`, :246-254 the inverse in
 * `encode`, :286-330 `_compute_poe_posterior`).  A flow is n_blocks MADEs of n_hidden + 1 masked linear layers ([H,D], [H,H] ...,
 * [2D,H]; ReLU between; "sequential" degrees); the masks are computed from indices (deg(k) = k % (D - 1)), never read, and a masked
 * weight's value never reaches a result.  One block: u = (x - mu(x)) exp(-lv(x)); ladj -= sum_d lv_d; x' = flip(u).
 * fp32 FMA, fixed summation order, no atomics: bit-reproducible.  2 <= D <= MVK_MAF_MAX_DIM, 1 <= H <= MVK_MAF_MAX_DIM,
 * 1 <= n_hidden <= MVK_MAF_MAX_HIDDEN, 1 <= n_blocks <= MVK_MAF_MAX_BLOCKS, 1 <= M <= MVK_MAX_MODALITIES.
 * W, b (and dW, db): HOST arrays of M * n_blocks * (n_hidden + 1) device pointers, entry (m * n_blocks + block) * (n_hidden + 1) +
 * layer, each the torch layout [out, in] / [out]; copied into the launch (capturable, nothing is repacked).
 * fwd: z [B,D] (shared by the M flows) -> z0 [M,B,D], ladj [M,B]; with mu0, lv0 (HOST arrays of M device pointers, [B,D] each; both
 * or neither, and `rows` with them) also rows[m,b] = -( sum_l log N(z0; mu0, exp(lv0 / 2)) + ladj ): JNF's stage-two row term.
 * ws (nullable: no backward will follow): M * n_blocks * B * (2 D + n_hidden H) floats; per (m, block) the block's input [B,D], its
 * lv [B,D] and the n_hidden hidden activations [B,H].
 * bwd: upstream grows [M,B] (needs mu0 / lv0), dz0 [M,B,D], dladj [M,B] (each nullable, at least one given), the forward's z0 and ws
 * -> dmu0[m], dlv0[m] [B,D] OVERWRITTEN (with mu0 / lv0); dz [B,D] (nullable) OVERWRITTEN with the sum over m in increasing m;
 * deltas (the size of ws; nullable when no weight gradient is wanted): the pre-activation gradients of every layer; dW, db
 * (nullable; a null ENTRY skips that tensor) +=, summed over b in increasing order by a second launch, masked entries untouched.
 * inverse (ONE flow: W, b hold n_blocks * (n_hidden + 1) pointers): y [R,D] -> x [R,D] with forward(x) = y, ladj [R] (nullable)
 * = sum of lv over blocks and coordinates (minus the forward's).
 * B = 0 / R = 0 is MVK_OK and writes nothing; a bad argument is MVK_EINVAL before any launch. */
#define MVK_MAF_MAX_DIM 512
#define MVK_MAF_MAX_HIDDEN 4
#define MVK_MAF_MAX_BLOCKS 4
int mvk_maf_fwd(const float* z, const float* const* W, const float* const* b, int M, int n_blocks, int n_hidden, int D, int H,
                const float* const* mu0, const float* const* lv0, int B, float* z0, float* ladj, float* rows, float* ws,
                void* stream);
int mvk_maf_bwd(const float* const* W, int M, int n_blocks, int n_hidden, int D, int H, const float* const* mu0,
                const float* const* lv0, const float* z0, const float* ws, const float* grows, const float* dz0,
                const float* dladj, int B, float* const* dmu0, float* const* dlv0, float* dz, float* deltas, float* const* dW,
                float* const* db, void* stream);
int mvk_maf_inverse(const float* y, const float* const* W, const float* const* b, int n_blocks, int n_hidden, int D, int H, int R,
                    float* x, float* ladj, void* stream);

/* Inverse autoregressive flow (IAF, models/nn/flows.py) for the flow samplers (samplers/iaf_sampler): ONE flow of the MADEs above
 * run the other way round, with the limits, pointer tables (n_blocks * (n_hidden + 1) entries), numeric contract, error codes and
 * B = 0 behaviour of mvk_maf_*.  With (m, s) = MADE(y), one block: y_i = (x_i - m_i(y)) exp(-s_i(y)) for i = 0..D-1 from y = 0,
 * ladj -= s_i; x' = flip(y).  The D steps cost ONE pass over the weights per block (the schedule of mvk_maf_inverse).
 * fwd: x [B,D] -> z0 [B,D], ladj [B]; rows [B] (nullable) = -( sum_d log N(z0_d; 0, 1) + ladj ), the flow's NLL row under N(0, I).
 * ws (nullable: no backward will follow): n_blocks * B * (2 D + n_hidden H) floats; per block the MADE's input y [B,D] (the block's
 * output before the flip), s [B,D] and the n_hidden hidden activations of MADE(y) [B,H].
 * bwd: upstream grows [B], dz0 [B,D], dladj [B] (each nullable, at least one given), the forward's z0 and ws -> dx [B,D] (nullable)
 * OVERWRITTEN; deltas (the size of ws; nullable when no weight gradient is wanted): the pre-activation gradients of every layer;
 * dW, db (nullable; a null ENTRY skips that tensor) +=, summed over b by the weight launch of mvk_maf_bwd.  The block's Jacobian in
 * y is lower triangular: one launch solves the transposed system coordinate by coordinate, interleaved with one MADE backward pass.
 * inverse: y [R,D] -> x [R,D] with forward(x) = y, ladj [R] (nullable): one MADE pass per block (y = flip(y), x = y exp(s) + m,
 * ladj += sum_d s_d). */
int mvk_iaf_fwd(const float* x, const float* const* W, const float* const* b, int n_blocks, int n_hidden, int D, int H, int B,
                float* z0, float* ladj, float* rows, float* ws, void* stream);
int mvk_iaf_bwd(const float* const* W, int n_blocks, int n_hidden, int D, int H, const float* z0, const float* ws,
                const float* grows, const float* dz0, const float* dladj, int B, float* dx, float* deltas, float* const* dW,
                float* const* db, void* stream);
int mvk_iaf_inverse(const float* y, const float* const* W, const float* const* b, int n_blocks, int n_hidden, int D, int H, int R,
                    float* x, float* ladj, void* stream);

/* MVAE (models/mvae/mvae_model.py:56-118): for each of the S subsets of the objective (subset_bits: HOST array, bit m
 * = modality m), the product of the AVAILABLE experts of the subset and the N(0,I) prior in the log-sum-exp form of
 * `stable_poe` (base_utils.py:133-147; a missing modality has log-variance +inf, mvae_model.py:71-75), one sample
 * z_s = mu_s + exp(lv_s / 2) eps[s] per row and kld_rows[s,b] = -1/2 sum_l (1 + lv_s - mu_s^2 - exp(lv_s)) (:100).
 * z_s is written into the decoder input of every modality of s: zm[m] is [K_m, B, L] with K_m = number of subsets
 * holding m, slab index = rank of s among them (HOST array of M device pointers; so each decoder runs once for all
 * its subsets).  eps [S,B,L]; sub_mu, sub_lv [S,B,L] optional outputs (both or neither).  Rows with no available
 * modality in s give the prior (kld 0, no gradient).  bwd: dzm[m] [K_m,B,L] (entries may be NULL), gkld_rows [S,B]
 * (nullable) -> dmu[m], dlv[m] [B,L] (overwritten). */
int mvk_mvae_posterior_fwd(const float* const* mu, const float* const* lv, const uint8_t* const* masks, int M,
                           const int32_t* subset_bits, int S, const float* eps, int B, int L, float* const* zm,
                           float* kld_rows, float* sub_mu, float* sub_lv, void* stream);
int mvk_mvae_posterior_bwd(const float* const* mu, const float* const* lv, const uint8_t* const* masks, int M,
                           const int32_t* subset_bits, int S, const float* eps, const float* const* dzm, int B, int L,
                           const float* gkld_rows, float* const* dmu, float* const* dlv, void* stream);

/* JMVAE (models/jmvae/jmvae_model.py:133-174): reparameterised sample(s) of the joint encoder's posterior
 * z[k] = joint_mu + exp(joint_lv/2) * eps[k], kld_rows[b] = KL(q(z|X) || N(0,I)) summed over L, and
 * ljm_rows[b] = sum_m KL(q(z|X) || q(z|x_m)) with (mu[m], lv[m]) the unimodal encoders' outputs.
 * bwd: gradients w.r.t. the joint and the unimodal parameters given dz [K,B,L] (may be NULL) and the per-row
 * gradients of the two KL terms (may be NULL = 0). */
int mvk_jmvae_posterior_fwd(const float* joint_mu, const float* joint_lv, const float* const* mu,
                            const float* const* lv, int M, const float* eps, int K, int B, int L, float* z,
                            float* kld_rows, float* ljm_rows, void* stream);
int mvk_jmvae_posterior_bwd(const float* joint_mu, const float* joint_lv, const float* const* mu,
                            const float* const* lv, int M, const float* eps, const float* dz, int K, int B, int L,
                            const float* gkld_rows, const float* gljm_rows, float* djoint_mu, float* djoint_lv,
                            float* const* dmu, float* const* dlv, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused reconstruction NLL over the K-sample axis
 * ------------------------------------------------------------------------------------------------ */
typedef struct mvk_recon_desc {
  const float* recon;   /* [K,B,D] decoder output (logits for bernoulli) */
  const float* x;       /* [B,D] target, broadcast over K */
  const uint8_t* mask;  /* [B] availability or NULL */
  float* rows;          /* out [K,B]: rescale * sum_d -log p(x|recon); NOT masked (fwd only) */
  float* drecon;        /* out [K,B,D] or NULL: coef * mask[b] * rowcoef[k,b] * rescale * d(-log p)/d recon */
  const float* rowcoef; /* [K,B] per-row gradient weight or NULL (= 1) */
  int64_t D;
  int32_t dist;         /* MVK_DIST_* */
  float scale;          /* normal / laplace scale */
  float rescale;        /* likelihood rescaling factor (base_ae_model.py:127-152) */
  float coef;           /* constant gradient weight (e.g. 1/(B*K)) */
  int32_t n_classes;    /* MVK_DIST_CATEGORICAL: size of the last (class) dimension, D % n_classes == 0; else ignored */
} mvk_recon_desc;

/* Per-(k,b) row NLL for up to MVK_MAX_MODALITIES modalities in ONE launch, optionally emitting
 * d(loss)/d(recon) in the same pass.  Replaces models/base/base_utils.py:62-87 (recon_log_probs) and the
 * `.view(B,-1).sum(-1)` row reductions of mopoe_model.py:192-199, mvtcae_model.py:60-68,
 * mmvae_model.py:208-214.  descs: HOST array. */
int mvk_recon_nll_fwd(const mvk_recon_desc* descs, int n_mod, int K, int B, void* stream);

/* Second pass for estimators whose row weights depend on a K-reduction (IWAE/DReG): writes drecon only. */
int mvk_recon_nll_bwd(const mvk_recon_desc* descs, int n_mod, int K, int B, void* stream);

/* Scalar assembly: out[i] = coef[i] * sum_j v_i[j] * (mask_i ? mask_i[j % period_i] : 1) for i < n_terms;
 * out[n_terms] = sum_i lossw[i] * out[i]; out[n_terms+1] = out[n_terms] * loss_sum_scale; *loss_out (nullable)
 * = out[n_terms].  n_terms <= MVK_MAX_TERMS.
 * Replaces the `.mean()` / `.sum()` / `loss = ...` lines of mopoe_model.py:200-227, mvtcae_model.py:96-108. */
#define MVK_MAX_TERMS 64
typedef struct mvk_term_desc {
  const float* v;
  const uint8_t* mask;
  int64_t n;
  int64_t period;
  float coef;
  float lossw;
  float* gfill; /* optional: gfill[0..n) = coef * lossw, the gradient of the loss w.r.t. this term's rows for an upstream
                 * gradient of 1 (terms that enter the loss as a plain weighted row sum: the KL rows) */
} mvk_term_desc;
int mvk_reduce_terms(const mvk_term_desc* terms, int n_terms, float loss_sum_scale, float* out, float* loss_out,
                     void* stream);
/* The same assembly on up to 32 workgroups of 256 threads (the one-workgroup form is latency-bound: 19 us alone for the 170 KB of row sums of
 * the headline step).  ws: caller-owned scratch of >= MVK_REDUCE_TERMS_WS_FLOATS floats whose FIRST word is an arrival counter
 * that must be 0 before the first launch and is 0 again after every launch; not shared between streams.  Every workgroup sums a
 * fixed slice of every term, the last one to arrive adds the partials in workgroup order: deterministic.  ws == NULL (or too
 * small, or no term longer than 4096 entries): exactly mvk_reduce_terms. */
#define MVK_REDUCE_TERMS_WS_FLOATS (1 + 32 * MVK_MAX_TERMS)
int mvk_reduce_terms_ws(const mvk_term_desc* terms, int n_terms, float loss_sum_scale, float* out, float* loss_out, float* ws,
                        int64_t ws_floats, void* stream);

/* buf[i] *= *gscale unless *gscale == 1 (no memory traffic in that case). */
int mvk_scale_by_device_scalar(float* buf, int64_t n, const float* gscale, void* stream);
/* Backward of the loss assembly in one launch (what autograd does for `loss = sum_i w_i * term_i` given d loss):
 * buffers with fill == 0 (the d loss / d recon tensors written by mvk_recon_nll_fwd for an upstream gradient of 1) are
 * multiplied in place by *gscale — skipped on the device when it is 1; buffers with fill != 0 (gradients of KL row
 * tensors) are set to *gscale * coef. */
#define MVK_SEED_MAX 12
typedef struct mvk_seed_desc {
  float* buf;
  int64_t n;
  float coef;
  int32_t fill;
} mvk_seed_desc;
int mvk_loss_backward_seed(const mvk_seed_desc* jobs, int n, const float* gscale, void* stream);

/* ------------------------------------------------------------------------------------------------
 * MMVAE: mixture-of-experts importance weights (IWAE / DReG)
 * ------------------------------------------------------------------------------------------------ */

/* std from log-variance: exp(lv/2), softmax(lv)*L + 1e-6 (models/mmvae/mmvae_model.py:66-74) or
 * softplus(lv) + 1e-6 (models/mmvaePlus/mmvaePlus_model.py:110-120) and its backward.  lv, std: [rows, L]. */
int mvk_mmvae_std_fwd(const float* lv, int rows, int L, int family, float* std, void* stream);
int mvk_mmvae_std_bwd(const float* lv, const float* std, const float* dstd, int rows, int L, int family,
                      float* dlv, void* stream);

/* For every conditioning modality c: z[c] = loc + std * t(noise) (Normal: t = n; Laplace: t = -sign(u) log1p(-|u|),
 * u ~ U(eps-1,1), torch.distributions.Laplace.rsample), lpz[c][k,b] = sum_l log p(z), lq_all[c][m,k,b] =
 * sum_l log q_m(z) (-inf where mask_m[b] == 0) and lqz[c][k,b] = logsumexp_m lq_all - log n_avail[b]
 * (mmvae_model.py:111-123, :160-206).  mu, std [B,L]; noise, z [K,B,L]; lpz, lqz [K,B]; lq_all [M,K,B]:
 * HOST arrays of M device pointers.  prior_mean, prior_std: device [L].  masks: HOST array of M uint8 [B]
 * device pointers (entries may be NULL) or NULL.
 *
 * MMVAE+ (mmvaePlus_model.py:122-262): the latent of a modality is [u (shared_dims), w (L - shared_dims)]; only the
 * first shared_dims dimensions enter the mixture (lq_all, lqz), the rest is scored by the conditioning modality's own
 * posterior: lqw[c][k,b] = sum_{l >= shared_dims} log q_c(z).  MMVAE: shared_dims = L, lqw = NULL.
 *
 * Common to the three mvk_mmvae_latent_* / mvk_mmvae_objective_fwd entry points:
 *   - 1 <= M <= MVK_MAX_MODALITIES, K >= 1, 1 <= shared_dims <= L, family NORMAL or LAPLACE_SOFTMAX;
 *   - B == 0 is a no-op that returns MVK_OK: nothing is launched and no output is written, the loss scalar of
 *     mvk_mmvae_objective_fwd included (the std and cross-latent entry points below treat rows == 0 the same way);
 *     B < 0 is MVK_EINVAL;
 *   - row indices are 32-bit: M * K * B must stay below 2^31 (MVK_EINVAL beyond); element offsets (times L) are 64-bit;
 *   - the masks must leave at least one modality present in every row: a row with none divides by n_avail = 0 and
 *     yields NaN, as the reference does. */
int mvk_mmvae_latent_fwd(const float* const* mu, const float* const* std, const float* const* noise,
                         const uint8_t* const* masks, const float* prior_mean, const float* prior_std, int M,
                         int K, int B, int L, int family, float* const* z, float* const* lpz,
                         float* const* lqz, float* const* lq_all, int shared_dims, float* const* lqw, void* stream);

/* lw[c] = (sum_r -rows[c][r] * mask_r + lpz[c] - lqz[c]) * mask_c, softmax weights w[c] over k, and
 * loss = -sum_b (1/n_avail[b]) sum_c obj_c[b] with obj = logsumexp_k lw - log K (IWAE) or sum_k w lw (DReG)
 * (mmvae_model.py:208-292).  rows: HOST array of M*M device pointers, rows[c*M + r] = [K,B] rescaled NLL rows
 * of modality r reconstructed from z[c] (mvk_recon_nll_fwd).  rowcoef[c] [K,B] = d loss / d lw[c] =
 * -w[c] mask_c / n_avail (the per-row weight of mvk_recon_nll_bwd).  loss: device scalar, overwritten. */
/* MMVAE+: lw[c] = (sum_r ... + beta * (lpz[c] - lqz[c] - lqw[c])) * mask_c (mmvaePlus_model.py:262); MMVAE passes
 * lqw = NULL, beta = 1. */
int mvk_mmvae_objective_fwd(const float* const* rows, const float* const* lpz, const float* const* lqz,
                            const uint8_t* const* masks, int M, int K, int B, int dreg, float* const* lw_out,
                            float* const* w, float* const* rowcoef, float* loss, const float* const* lqw, float beta,
                            void* stream);

/* Latent-side backward.  dz_dec[c] [K,B,L]: gradient of the loss w.r.t. z[c] through the decoders (from
 * mvk_recon_nll_bwd with rowcoef = -w[c]/n_avail and the decoders' own backward).  Produces dmu[c], dstd[c]
 * [B,L] and dprior_std [B,L] (nullable): the per-row terms of d loss / d prior_std, which the caller sums over the rows
 * (mvk_colsum_acc: fixed order, bit-reproducible).  DReG: q parameters are detached inside log q and the total gradient
 * reaching z is scaled by w once more (the hook of mmvae_model.py:263-266).  Rows b with mask_c[b] == 0 contribute nothing
 * for conditioning modality c: dz_dec[c][:, b, :] is not read there (mvk_recon_nll_bwd leaves it zero, rowcoef being 0). */
int mvk_mmvae_latent_bwd(const float* const* mu, const float* const* std, const float* const* noise,
                         const float* const* z, const uint8_t* const* masks, const float* prior_mean,
                         const float* prior_std, const float* const* w, const float* const* lq_all,
                         const float* const* lqz, const float* const* dz_dec, int M, int K, int B, int L,
                         int family, int dreg, const float* gscale, float* const* dmu, float* const* dstd,
                         float* dprior_std, int shared_dims, float beta,
                         void* stream);

/* MMVAE+ cross-modal decoder input (mmvaePlus_model.py:152-172): zc[r, :Ls] = z[r, :Ls] (the shared latent of the
 * conditioning modality) and zc[r, Ls + j] = prior_std[j] * t(noise[r, j]) (a reparameterised sample of the TARGET
 * modality's private prior, mean 0).  rows = K*B, z / zc [rows, D], noise [rows, D - Ls], prior_std [D - Ls].
 * bwd: dz [rows, D] (zero in the private dims) and dprior_std [D - Ls] (nullable), overwritten. */
int mvk_mmvaeplus_cross_latent_fwd(const float* z, const float* prior_std, const float* noise, int64_t rows, int D,
                                   int Ls, int family, float* zc, void* stream);
int mvk_mmvaeplus_cross_latent_bwd(const float* dzc, const float* noise, int64_t rows, int D, int Ls, int family,
                                   float* dz, float* dprior_std, void* stream);

/* ------------------------------------------------------------------------------------------------
 * CMVAE (models/cmvae/cmvae_model.py): MMVAE+ with a learnable mixture over C clusters as the prior of the shared latent.
 * The reference's explicit expectation over q(c|u) = softmax_c(a_c) + 1e-20, a_c = log pi_c + log p(u|c) (:292-337), is
 * evaluated in closed form: sum_c q_c (a_c - log q_c) = logsumexp_c a_c.
 * ------------------------------------------------------------------------------------------------ */

/* The cluster table (means, stds, log pi) of a launch is staged in LDS: 1 <= C <= MVK_CMVAE_MAX_CLUSTERS and
 * C * (2 * (Ls | 1) + 1) + 4 * Ls <= MVK_CMVAE_MAX_LDS_FLOATS (the 4 * Ls: mvk_cmvae_latent_fwd only), MVK_EINVAL beyond.
 * C = 64 fits up to Ls = 91, C = 128 up to Ls = 45, C = 10 up to Ls = 511.
 * At least one entry of cluster_logits must be finite: with every logit at -inf the softmax is 0 / 0 and lpz, resp and pc_z are
 * NaN, as torch.softmax of the same logits is (CMVAE.prune_clusters stops at two clusters and never gets there). */
#define MVK_CMVAE_MAX_CLUSTERS 128
#define MVK_CMVAE_MAX_LDS_FLOATS 12288

/* The latent stage of mvk_mmvae_latent_fwd for the MMVAE+ layout [u (shared_dims = Ls < D), w (D - Ls)], ONE launch, same
 * arguments, conventions (B == 0, M * K * B < 2^31, masks) and outputs z, lqz, lq_all, lqw, with the prior replaced by
 *   lpz[c][k,b] = logsumexp_j(log_softmax(cluster_logits)_j + sum_{l < Ls} log p(u_l; cluster_mean[j,l], cluster_std[j,l]))
 *                 + sum_{l >= Ls} log p(w_l; 0, wprior_std[l - Ls])
 * and resp[c][k,b,j] = the softmax over j of the same terms (no 1e-20), which the backward launch reads.  cluster_mean,
 * cluster_std: device [C, Ls]; cluster_logits: device [C] (log pi is computed in the launch; a logit of -inf makes the
 * cluster absent: zero responsibility, no NaN, where the reference's literal form gives -inf through 1e-20 * -inf);
 * wprior_std: device [D - Ls]; resp: HOST array of M device pointers [K,B,C]; lqw is required. */
int mvk_cmvae_latent_fwd(const float* const* mu, const float* const* std, const float* const* noise,
                         const uint8_t* const* masks, const float* cluster_mean, const float* cluster_std,
                         const float* cluster_logits, const float* wprior_std, int M, int K, int B, int D, int family,
                         int C, float* const* z, float* const* lpz, float* const* lqz, float* const* lq_all,
                         int shared_dims, float* const* lqw, float* const* resp, void* stream);

/* Latent-side backward, ONE launch with the per-b ownership of mvk_mmvae_latent_bwd (dmu, dstd [B,D] summed over c and k in a
 * fixed order, no atomics).  The prior's pull on u is coef * beta * sum_j resp_j * d log p(u; mean_j, std_j) / du.
 * dparams [B, C * Ls + C] (overwritten): row b holds the terms of batch row b of d loss / d cluster_mean ([C, Ls], entry
 * (j, l) = coef * beta * resp_j * d log p / d mean_jl) followed by d loss / d cluster_logits ([C], entry i = coef * beta *
 * (resp_i - pi_i)); the caller sums the rows with one mvk_colsum_acc.  coef = d loss / d lw = -gscale * w / n_avail, IWAE and
 * DReG alike: under DReG only the path through the reparameterised sample takes w a second time (as dprior_std in
 * mvk_mmvae_latent_bwd).  The cluster stds and wprior_std get no gradient (the reference fixes them). */
int mvk_cmvae_latent_bwd(const float* const* mu, const float* const* std, const float* const* noise,
                         const float* const* z, const uint8_t* const* masks, const float* cluster_mean,
                         const float* cluster_std, const float* cluster_logits, const float* wprior_std,
                         const float* const* w, const float* const* lq_all, const float* const* lqz,
                         const float* const* resp, const float* const* dz_dec, int M, int K, int B, int D, int family,
                         int dreg, int C, const float* gscale, float* const* dmu, float* const* dstd, float* dparams,
                         int shared_dims, float beta, void* stream);

/* predict_clusters (:546-619) for R rows z [R, Ls], ONE launch: pc_z [C, R] = softmax_j(log(softmax(cluster_logits)_j + 1e-20)
 * + sum_l log p(z_l; cluster_mean[j,l], cluster_std[j,l])) (here the reference does add 1e-20 inside the log: a pruned cluster
 * has log 1e-20, not -inf), argmax [R] (int64) = the first maximum of pc_z[:, r], norm_llik [R] (nullable) =
 * sum_j pc_j (lpz_j + lpc_j - log pc_j) / Ls, evaluated as logsumexp_j(lpc_j + lpz_j) / Ls (finite where pc_j underflows to 0
 * and the literal form is 0 * inf).  R == 0 returns MVK_OK without a launch; R < 2^31. */
int mvk_cmvae_assign(const float* z, const float* cluster_mean, const float* cluster_std, const float* cluster_logits,
                     int64_t R, int Ls, int family, int C, float* pc_z, int64_t* argmax, float* norm_llik,
                     void* stream);

/* ------------------------------------------------------------------------------------------------
 * Importance-sampled joint likelihood (compute_joint_nll; metrics/likelihoods/likelihoods.py:39-56 is the caller)
 * ------------------------------------------------------------------------------------------------ */

/* z[k,b,:] = loc[b,:] + sd[b,:] * t(noise[k,b,:]) (t as in mvk_mmvae_latent_fwd): the K importance samples of every
 * data point, `rsample_from_gaussian(mu, lv, N=K)` (base_utils.py:150-172) / `post_dist(mu, sd).rsample([K])`.
 * loc, sd [B,L]; noise, z [K,B,L]. */
int mvk_iwae_sample(const float* loc, const float* sd, const float* noise, int K, int B, int L, int family, float* z,
                    void* stream);

/* lw[k,b] = -sum_r rows[r][k,b] + sum_l log p(z[k,b,l]) - (logsumexp_e sum_l log q_e(z[k,b,l]) - log E)
 * with q_e = family(loc[e][b,:], sd[e][b,:]) and the prior family(prior_loc, prior_sd) (NULL: 0 / 1).  Replaces the
 * per-data-point, per-chunk bodies of mopoe_model.py:524-588, mmvae_model.py:400-437, mvtcae_model.py:250-284 and
 * joint_model.py:113-148.  rows: HOST array of n_rows device pointers to [K,B] UNRESCALED NLL rows
 * (mvk_recon_nll_fwd with rescale = 1); loc, sd: HOST arrays of E <= MVK_IWAE_MAX_EXPERTS device pointers [B,L];
 * z [K,B,L]; lw [K,B].  Non-finite densities follow torch.logsumexp: an expert at -inf drops out of the mixture, all experts at
 * -inf give lw = +inf, and a NaN expert density (sd = 0) gives lw = NaN for that (k,b). */
int mvk_iwae_logw(const float* z, const float* const* rows, int n_rows, const float* const* loc,
                  const float* const* sd, int E, const float* prior_loc, const float* prior_sd, int K, int B, int L,
                  int family, float* lw, void* stream);

/* ll[b] = logsumexp over the n arrays lw[j][k,b] (k < K) - log(n K): the log-mean-exp of the importance weights
 * (the two-level logsumexp over K-chunks of the reference is the same number; MMVAE+ concatenates the weights of its
 * M conditioning modalities, mmvaePlus_model.py:521-525).  lw: HOST array of n <= MVK_MAX_MODALITIES device
 * pointers [K,B]; ll [B].  As torch.logsumexp: a column that is all -inf gives -inf, a +inf entry gives +inf, a NaN entry NaN. */
int mvk_iwae_reduce(const float* const* lw, int n, int K, int B, float* ll, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Encoder / decoder layers: implicit GEMM with fp32 operands and results.  Default engine: split-bf16 MFMA
 * (3 bf16 pieces per operand, 6 piece products, fp32 accumulate: fp32-level error); MVK_ENGINE=f32 selects
 * v_mfma_f32_32x32x2_f32 (exact fp32 FMA chains), which also serves small / irregular shapes.
 * ------------------------------------------------------------------------------------------------ */

/* Y[M,N] = act(X[M,K] W[N,K]^T + b[N]) — nn.Linear + activation
 * (models/nn/default_architectures.py:21-72 Encoder_VAE_MLP, :225-258 Decoder_AE_MLP). */
int mvk_linear_fwd(const float* X, const float* W, const float* b, float* Y, int M, int N, int K, int act,
                   float* ws, int64_t ws_floats, void* stream);
/* dX[M,K] = dYpre[M,N] W[N,K] (* act'(prev_out[m,k]) if prev_out != NULL, so the result is directly the
 * previous layer's pre-activation gradient).  dYpre = dY * act'(y_out) when y_out != NULL, else dY.
 * accumulate != 0: dX += (atomic).
 * colsum_acc (may be NULL; requires accumulate == 0): colsum_acc[k] += sum_m dX[m,k] — the previous layer's bias
 * gradient, fused into this launch's epilogue. */
int mvk_linear_bwd_data(const float* dY, const float* W, float* dX, int M, int N, int K, const float* y_out,
                        int y_act, const float* prev_out, int prev_act, int accumulate, float* colsum_acc,
                        float* ws, int64_t ws_floats, void* stream);
/* dW[N,K] += dYpre[M,N]^T X[M,K];  db[N] += colsum(dYpre) (db nullable).
 * Split-K workspace convention (all weight-gradient / accumulate entry points): `ws` is caller-owned scratch of
 * `ws_floats` floats.  When it can hold one [rows x cols] slab per reduction slice the slices are summed by a
 * second kernel in a fixed order (deterministic, no atomics); with ws == NULL or too small the slices fall
 * back to fp32 atomicAdd.  mvk_splitk_workspace_floats() returns a size that is always sufficient. */
int mvk_linear_bwd_weight(const float* dY, const float* X, float* dW, float* db, int M, int N, int K,
                          const float* y_out, int y_act, float* ws, int64_t ws_floats, void* stream);
int64_t mvk_splitk_workspace_floats(int rows, int cols, int reduce_len);
/* dPre[M,N] = dY * act'(Y) and, if db != NULL, db[n] += sum_m dPre[m,n], in one pass over dY and Y (ordered
 * per-workgroup partials in the caller-owned scratch ws).  The output-layer backward of the MLP decoders. */
int mvk_act_bwd_colsum(const float* dY, const float* Y, int act, int M, int N, float* dPre, float* db, float* ws,
                       int64_t ws_floats, void* stream);
/* db[N] += column sums of dY[M,N] (* act'(y_out)): per-workgroup partials in the caller-owned scratch ws, summed in a
 * fixed order (bit-reproducible); ws == NULL (or too small) falls back to fp32 atomics. */
int mvk_colsum_acc(const float* dY, const float* y_out, int y_act, float* db, int M, int N, float* ws, int64_t ws_floats,
                   void* stream);
/* db[c] += sum over n and spatial positions of dY[n,c,hw] (* act'(y_out)) for NCHW tensors. */
int mvk_nchw_channel_sum_acc(const float* dY, const float* y_out, int y_act, float* db, int n, int c, int hw,
                             float* ws, int64_t ws_floats, void* stream);
/* In-place dY *= act'(Y) (sigmoid: y(1-y), relu: y>0). */
int mvk_act_bwd(float* dY, const float* Y, int64_t n, int act, void* stream);
/* out = a * g * act'(Y) in one pass (out may alias g): the gradient through `a * act(.)`, e.g. the 0.1 of a ResNet block's
 * residual branch and the activation behind its second convolution (models/nn/mmnist.py:229-246). */
int mvk_act_bwd_scaled(const float* g, float a, const float* Y, int act, float* out, int64_t n, void* stream);

/* Row-major GEMM C[M,N] (+)= op(A) op(B) used for the packed 1x1-spatial layers:
 *   ta=0: A is [M,K]; ta=1: A is [K,M].  tb=0: B is [K,N]; tb=1: B is [N,K].
 *   bias[n % bias_mod] added when bias != NULL; act applied; a_act_src: A *= a_act'(a_act_src) on load;
 *   c_act_src: result *= c_act'(c_act_src[m,n]); accumulate != 0 => C += (split-K, atomic). */
int mvk_gemm(const float* A, const float* B, float* C, int M, int N, int K, int ta, int tb, const float* bias,
             int bias_mod, int act, int accumulate, const float* a_act_src, int a_act, const float* c_act_src,
             int c_act, float* ws, int64_t ws_floats, void* stream);

/* Pre-split ("bf3") tensor format of the split-bf16 GEMM engine: x = p0 + p1 + p2 with p0 = bf16(x),
 * p1 = bf16(x - p0), p2 = bf16(x - p0 - p1) (round to nearest); stored as three planes of n bf16 values,
 * plane i at byte offset i * 2 * n.  A producer writes it once; every consuming GEMM saves the per-k-tile split. */
#define MVK_FMT_IN_BF3 1
/* mvk_conv4s2_up only: take the tiled engine (three resident workgroups of <= 128 registers per SIMD) even where the
 * register-stationary kernel (one 512-register wave per SIMD) covers the shape — for a launch that has to run BESIDE such a
 * kernel of another stream instead of behind it (the convolutional encoder's backward-data launches in the step's tail). */
#define MVK_FMT_TILED 2
int mvk_f32_to_bf3(const float* x, int64_t n, void* planes, void* stream);
int mvk_bf3_to_f32(const void* planes, int64_t n, float* x, void* stream);

/* 4x4 / stride 2 / pad 1 convolution pair on NHWC activations (models/nn/svhn.py:7-70).
 * "U" is the large feature map [n,2h,2w,Cu], "V" the small one [n,h,w,Cv], W the reference weight
 * tensor indexed [Cv][Cu][4][4] (nn.Conv2d weight [out,in,kh,kw] with V = output; nn.ConvTranspose2d
 * weight [in,out,kh,kw] with V = input).
 *   pack:  Wdown[(kh*4+kw)*Cu + cu][col_off + cv] (row stride ld_down) and/or
 *          Wup[ph*2+pw][((a*2+b)*Cv + cv)][cu], kh = (1-ph)+2a, kw = (1-pw)+2b
 *   down:  V = act(conv(U) + b) (* v_act'(v_act_src))   — Conv2d forward / ConvTranspose2d backward-data
 *   up:    U = act(convT(V) + b) (* u_act'(u_act_src))  — ConvTranspose2d forward / Conv2d backward-data
 *   wgrad: dWref[Cv][Cu][4][4] += sum_pos U(gathered) V — both layer types
 * u_nchw != 0: U is stored NCHW (network input / output boundary tensors only).
 * u_act_src (down, wgrad): U is a gradient tensor that is multiplied by u_act'(u_act_src) while loading.
 * fmt (down, up): MVK_FMT_IN_BF3 — the gathered input (U for down, V for up) is a pre-split tensor (see
 *   mvk_f32_to_bf3): three bf16 planes [3][n*H*W*C]; the GEMM then stages it without any conversion work.
 * colsum_acc (down, up; may be NULL): colsum_acc[c] += sum over positions of the stored output — the bias gradient
 *   of the layer whose output gradient this launch produces (replaces a separate pass over that tensor; uses the
 *   caller-owned scratch ws for per-workgroup partials, reduced in a fixed order). */
int mvk_pack_conv4s2_weight(const float* Wref, int Cv, int Cu, float* Wdown, int ld_down, int col_off,
                            float* Wup, void* stream);
/* All weight packs of one network in ONE launch.  kind 0: as mvk_pack_conv4s2_weight (Wdown and/or Wup, ld_down
 * <= 0 means Cv); kind 1: as mvk_pack_unflatten_weight with Cv = Cin, Cu = Cout, destination in Wup; kind 2: 3x3
 * convolution weight Wref[Cv = Cout][Cu = Cin][3][3] -> Wdown[(tap*Cu + cu)][cv] (forward operand of mvk_conv3x3) and/or
 * Wup[((8-tap)*Cv + cv)][cu] (its backward-data operand: flipped window, channels swapped). */
#define MVK_PACK_MAX 16
typedef struct mvk_pack_desc {
  const float* Wref;
  float* Wdown;
  float* Wup;
  int Cv, Cu, ld_down, col_off, kind;
  void* Fdown; /* kind 0, optional: the weights as bf16-piece MFMA fragments in the order the register-stationary */
  void* Fup;   /* convolution kernels (csrc/imgconv.hip) load them: [role][k-step 16][piece 3][lane 64][8 bf16],  */
               /* mvk_imgconv_frag_bytes(Cu, Cv) bytes each; passed to mvk_conv4s2_down / _up as `wfrag` */
  float* amax; /* optional: receives max |Wref| (atomic max: must hold 0 before the launch) — the w_amax of mvk_conv3x3_s */
} mvk_pack_desc;
int64_t mvk_imgconv_frag_bytes(int Cu, int Cv); /* 0: this channel pair has no register-stationary kernel */
int mvk_pack_weights(const mvk_pack_desc* jobs, int n, void* stream);
int mvk_conv4s2_down(const float* U, const float* Wdown, const float* bias, float* V, int n, int h, int w,
                     int Cu, int Cv, int act, int u_nchw, const float* u_act_src, int u_act,
                     const float* v_act_src, int v_act, float* colsum_acc, float* ws, int64_t ws_floats, int fmt,
                     const void* wfrag, void* stream);
int mvk_conv4s2_up(const float* V, const float* Wup, const float* bias, float* U, int n, int h, int w, int Cu,
                   int Cv, int act, int u_nchw, const float* u_act_src, int u_act, float* colsum_acc, float* ws,
                   int64_t ws_floats, int fmt, const void* wfrag, void* stream);
/* The two launches above on the register-stationary kernels (csrc/imgconv.hip) with the amax protocol of mvk_conv3x3_s: x_amax
 * + w_amax (both or neither) select the scaled-fp16 form (3 fp16 MFMAs per product instead of 6 bf16 ones; the weights are
 * converted in the kernel from the fp32 pack Wdown / Wup, whose max |w| the `amax` slot of mvk_pack_weights delivers), y_amax
 * (optional, zeroed) receives max |result| for the launch that consumes it.  NHWC tensors, no fused input activation.
 * mvk_conv4s2_scaled_ok: 1 when the layer pair and the batch are covered (else both return MVK_EINVAL). */
/* Two producers of the SVHN decoder that publish the maximum of what they write (so that the layer behind them can take the
 * scaled-fp16 form without a pass over the tensor): the short-reduction first layer and the fused-tail backward of the image
 * layer.  Same arguments as mvk_gemm (ta = 0, no fused operand activations) / mvk_conv4s2_small_up_bwd_pre. */
int mvk_gemm_smallk_amax(const float* A, const float* B, float* C, int M, int N, int K, int tb, const float* bias, int bias_mod,
                         int act, float* y_amax, void* stream);
int mvk_conv4s2_small_up_bwd_pre_y(const float* dpre, const float* rowscale, const float* V, int v_act, const float* Wref,
                                   float* dV, float* dWref, float* db, float* db_v, float* ws, int64_t ws_floats, int n, int h,
                                   int w, int Cu, int Cv, float* dv_amax, void* stream);
int mvk_conv4s2_scaled_ok(int n, int h, int w, int Cu, int Cv);
/* mvk_conv4s2_wgrad on scaled fp16 pairs (one accumulator per tile; V carries the 2^11 between main and cross terms in a third
 * piece): u_amax / v_amax = device scalars >= max |U| / max |V|.  NHWC U, no fused activation. */
int mvk_conv4s2_wgrad_scaled_ok(int n, int h, int w, int Cu, int Cv);
int mvk_conv4s2_wgrad_s(const float* U, const float* V, float* dWref, int n, int h, int w, int Cu, int Cv, const float* u_amax,
                        const float* v_amax, float* ws, int64_t ws_floats, void* stream);
int mvk_conv4s2_down_s(const float* U, const float* Wdown, const float* bias, float* V, int n, int h, int w, int Cu, int Cv,
                       int act, const float* v_act_src, int v_act, float* colsum_acc, const float* x_amax,
                       const float* w_amax, float* y_amax, float* ws, int64_t ws_floats, const void* wfrag, void* stream);
int mvk_conv4s2_up_s(const float* V, const float* Wup, const float* bias, float* U, int n, int h, int w, int Cu, int Cv,
                     int act, const float* u_act_src, int u_act, float* colsum_acc, const float* x_amax, const float* w_amax,
                     float* y_amax, float* ws, int64_t ws_floats, const void* wfrag, void* stream);
int mvk_conv4s2_wgrad(const float* U, const float* V, float* dWref, int n, int h, int w, int Cu, int Cv,
                      int u_nchw, const float* u_act_src, int u_act, float* ws, int64_t ws_floats, void* stream);
/* Two of those in ONE launch: the weight gradients of two 4x4 / stride-2 layers of one network at the same batch (the two inner
 * layers of Encoder_VAE_SVHN, models/nn/svhn.py:19-28, at the training batch, where each is a split-K GEMM of ~35 us on the
 * step's last dependent chain).  Both problems' workgroups share one grid (igemm_bf_pair_kernel); slabs and ordered finishes are
 * those of two separate mvk_conv4s2_wgrad launches (bit-identical gradients); shapes the pair launch does not cover run as two
 * launches.  NHWC U, no fused activation.  */
int mvk_conv4s2_wgrad_pair(const float* U0, const float* V0, float* dW0, int h0, int w0, int Cu0, int Cv0, const float* U1,
                           const float* V1, float* dW1, int h1, int w1, int Cu1, int Cv1, int n, float* ws, int64_t ws_floats,
                           void* stream);

/* 3x3 / stride 1 / pad 1 convolution on NHWC activations — the ResNet blocks of models/nn/mmnist.py:214-366 and
 * models/nn/cub.py:144-293.  Y[n,H,W,Cout] = act(conv(X[n,H,W,Cin]) + bias) (* src_act'(y_act_src) elementwise), with
 * Wp the kind-2 pack of mvk_pack_weights.  Backward data is the same launch on the output gradient with the Wup pack
 * (Cin / Cout swapped); colsum_acc as in mvk_conv4s2_down.  wgrad: dWref[Cout][Cin][3][3] += sum_pos X(gathered) dY. */
int mvk_conv3x3(const float* X, const float* Wp, const float* bias, float* Y, int n, int H, int W, int Cin, int Cout,
                int act, const float* y_act_src, int y_src_act, float* colsum_acc, float* ws, int64_t ws_floats,
                void* stream);
/* The same launch with a residual in the epilogue: Y = res + res_alpha * (act(conv(X) + bias) * src_act'(y_act_src)) —
 * `xs + 0.1 * conv2(...)` of the ResNet blocks (models/nn/cub.py:274-280) and `d_block_input + d_shortcut` of their backward
 * pass in one pass over the output. */
int mvk_conv3x3_res(const float* X, const float* Wp, const float* bias, float* Y, int n, int H, int W, int Cin,
                    int Cout, int act, const float* y_act_src, int y_src_act, const float* res, float res_alpha,
                    float* ws, int64_t ws_floats, void* stream);
int mvk_conv3x3_wgrad(const float* X, const float* dY, float* dWref, int n, int H, int W, int Cin, int Cout,
                      float* ws, int64_t ws_floats, void* stream);
/* Fused forms of the three launches above, taken only by the register-stationary kernels (csrc/conv3rs.hip); they fold the
 * elementwise passes of a ResnetBlock (models/nn/cub.py:274-280 `x_s + 0.1 * conv_1(actvn(conv_0(actvn(x))))`, mmnist.py:229-246)
 * into the convolutions on either side:
 *   mvk_conv3x3_fused_ok   1 when both fused launches take this problem (ask first: they return MVK_EINVAL otherwise)
 *   mvk_conv3x3_f          Y = [res + res_alpha *] (act(pre_scale * conv(x_act(X)) + bias) * src_act'(y_act_src)): x_act is the
 *                          activation of the layer that produced X, applied while X is staged (the activated tensor is never
 *                          written); res may be NULL; colsum_acc as in mvk_conv3x3 (backward-data form, exclusive with res)
 *   mvk_conv3x3_wgrad_f    dWref += dy_scale * sum_pos x_act(X)(gathered) dY and, when db != NULL, db[Cout] += dy_scale * sum_pos dY
 *                          (the bias gradient without a pass of its own; dy_scale = the 0.1 of the residual branch) */
int mvk_conv3x3_fused_ok(int n, int H, int W, int Cin, int Cout);
int mvk_conv3x3_f(const float* X, const float* Wp, const float* bias, float* Y, int n, int H, int W, int Cin, int Cout,
                  int act, const float* y_act_src, int y_src_act, const float* res, float res_alpha, float* colsum_acc,
                  int x_act, float pre_scale, float* ws, int64_t ws_floats, void* stream);
int mvk_conv3x3_wgrad_f(const float* X, const float* dY, float* dWref, float* db, int n, int H, int W, int Cin, int Cout,
                        int x_act, float dy_scale, float* ws, int64_t ws_floats, void* stream);
/* Scaled-fp16 form of mvk_conv3x3_f: every fp32 product is 3 fp16 MFMAs (hi hi' + (hi lo' + lo hi') / 2048, error-corrected
 * fp16 pairs after Ootomo & Yokota 2022; csrc/bf3.hpp states the error bound) instead of the 6 bf16 ones.  fp16 has a narrow
 * exponent, so each operand tensor is scaled by a power of two taken from an UPPER BOUND of its largest magnitude:
 *   x_amax, w_amax  device scalars >= max |X|, max |Wp| (finite inputs; a bound that is too small overflows to inf)
 *   y_amax          optional: max |Y| of this launch lands here by atomic max (*y_amax must hold 0 before the launch) and
 *                   can be the x_amax of the launch that consumes Y
 * mvk_amax computes the bound of any tensor (same protocol: *out holds 0 or a lower bound to keep); mvk_pack_weights fills
 * the `amax` slot of a descriptor.  mvk_conv3x3_scaled_ok: 1 when this form takes the problem (a superset of the shapes of
 * mvk_conv3x3_fused_ok's forward side: 128 input channels reach maps up to 62 wide). */
int mvk_amax(const float* x, int64_t n, float* out, void* stream);
/* mvk_conv3x3 with an image (Cin <= 4) on the input side that also publishes max |Y| into y_amax (atomic max, must hold 0):
 * conv_img of the ResNet encoders (models/nn/mmnist.py:262, cub.py:160) and the backward-data pass of the decoders' conv_img —
 * the stack behind it needs that bound for its scaled-fp16 launches and used to get it from a pass over Y (mvk_amax).
 * MVK_EINVAL when the direct image kernel does not take the shape (the caller then uses mvk_conv3x3 + mvk_amax). */
int mvk_conv3x3_y(const float* X, const float* Wp, const float* bias, float* Y, int n, int H, int W, int Cin, int Cout, int act,
                  const float* y_act_src, int y_src_act, float* colsum_acc, float* y_amax, float* ws, int64_t ws_floats,
                  void* stream);
int mvk_conv3x3_scaled_ok(int n, int H, int W, int Cin, int Cout);
int mvk_conv3x3_s(const float* X, const float* Wp, const float* bias, float* Y, int n, int H, int W, int Cin, int Cout,
                  int act, const float* y_act_src, int y_src_act, const float* res, float res_alpha, float* colsum_acc,
                  int x_act, float pre_scale, const float* x_amax, const float* w_amax, float* y_amax, float* ws,
                  int64_t ws_floats, void* stream);
/* mvk_conv3x3_s in its residual form with a second store (round 5): Y <- res + res_alpha * a and y_pre <- a, a = act(conv + bias).
 * The post-activation ResnetBlock of models/nn/mmnist.py:229-246 (x_s + 0.1 * lrelu(conv2(.))) keeps `a` for its backward pass:
 * one launch instead of the convolution and an elementwise pass over three tensors.  Where mvk_conv3x3_scaled_ok says so. */
int mvk_conv3x3_s2(const float* X, const float* Wp, const float* bias, float* Y, float* y_pre, int n, int H, int W, int Cin, int Cout,
                   int act, const float* res, float res_alpha, const float* x_amax, const float* w_amax, float* y_amax, float* ws,
                   int64_t ws_floats, void* stream);
/* One launch of mvk_conv3x3_s over a SLICE of the layer's input channels (round 5): X [n][H][W][x_channels], the slice = Cin
 * channels from x_off; Wp = the layer's whole pack [9 x_channels][Cout].  res_pre != 0: Y = act(conv + bias + res), `res` = the
 * partial sum the other slice's launch left (act = none, no bias there).  The register-stationary kernels hold the weights of at
 * most 128 input channels: a 256-channel layer (models/nn/mmnist.py:345-352, cub.py:233-240) is two such launches. */
int mvk_conv3x3_s_part(const float* X, int x_channels, int x_off, const float* Wp, const float* bias, float* Y, int n, int H, int W,
                       int Cin, int Cout, int act, const float* y_act_src, int y_src_act, const float* res, int res_pre, int x_act,
                       float pre_scale, const float* x_amax, const float* w_amax, float* y_amax, void* stream);
/* mvk_conv3x3_wgrad_f on scaled fp16 pairs (one accumulator per tap tile: the 2^11 between main and cross terms sits in a
 * third piece of dY, csrc/conv3rs.hip); x_amax / dy_amax: device scalars >= max |X| / max |dY|. */
int mvk_conv3x3_wgrad_scaled_ok(int n, int H, int W, int Cin, int Cout);
int mvk_conv3x3_wgrad_s(const float* X, const float* dY, float* dWref, float* db, int n, int H, int W, int Cin, int Cout,
                        int x_act, float dy_scale, const float* x_amax, const float* dy_amax, float* ws, int64_t ws_floats,
                        void* stream);
/* nn.AvgPool2d(3, stride=2, padding=1) (count_include_pad: every window divides by 9) and nn.Upsample(scale_factor=2)
 * (nearest) on NHWC tensors, forward and backward; out = act(a*x + b*y) (x or y may be NULL). */
int mvk_avgpool3s2_fwd(const float* x, float* y, int n, int H, int W, int C, void* stream);
int mvk_avgpool3s2_bwd(const float* dy, float* dx, int n, int H, int W, int C, void* stream);
int mvk_upsample2_fwd(const float* x, float* y, int n, int H, int W, int C, void* stream);
int mvk_upsample2_bwd(const float* dy, float* dx, int n, int H, int W, int C, void* stream);
int mvk_axpby(const float* x, float a, const float* y, float b, int64_t n, int act, float* out, void* stream);
/* Measurement aid of bench.py (not on the training path): one launch of a register-only loop of v_mfma_f32_32x32x16_bf16 — 256
 * workgroups, one wave per SIMD, 4 accumulator chains, 64 * iters MFMAs per chain — with hashed operand values (random_operands = 1)
 * constants (0), or hashed fp16 values on v_mfma_f32_32x32x16_f16 (2: the scaled-fp16 kernels' instruction).  Timed by the caller, it gives the matrix-pipe rate the chip SUSTAINS for a launch of that length; with
 * realistic operands that is 1.4-1.9 PFLOP/s, not the 2.5 of the data sheet (power-limited clock).  out: >= 65536 floats. */
int mvk_probe_mfma_bf16(float* out, int iters, int random_operands, void* stream);
/* Measurement aid of bench.py: a float4 streaming copy of n floats (16-byte aligned, n % 4 == 0; nontemporal, four loads in
 * flight per lane) — the measured HBM denominator beside the 8 TB/s of the data sheet. */
int mvk_probe_stream_copy(float* dst, const float* src, int64_t n, void* stream);
/* y[b][c][r] = act(x[b][r][c]) * dact'(msrc[b][r][c]) (msrc may be NULL; the derivative is taken through the OUTPUT of dact,
 * as everywhere here): the NCHW flatten in front of `fc_mu / fc_logvar` of the ResNet encoders fused with their last activation
 * (models/nn/cub.py:190-195, mmnist.py:300-306), the un-flatten behind `fc` of the decoders (cub.py:232-240), and their
 * backward passes — x, msrc: [batch][rows][cols], y: [batch][cols][rows]; batch <= 65535. */
int mvk_transpose_act(const float* x, float* y, int batch, int rows, int cols, int act, const float* msrc, int dact,
                      void* stream);

/* Noise drawn with the generator state in device memory (the reparameterisation noise of models/base/base_utils.py:129-160
 * `rsample_from_gaussian` and of every `rsample` on the path; the reference calls torch's generator).  state: 3 x uint64
 * {seed, offset, arrival ticket} owned by the caller, advanced by the launch itself — a captured training step draws fresh
 * noise at every replay with no host-issued launch in front of it.  Philox4x32-10, counter = offset + index / 4; uniform = 0:
 * N(0, 1) by Box-Muller; uniform = 1: U[lo, hi).  The values depend only on (seed, offset, index). */
int mvk_device_rng(float* out, int64_t n, uint64_t* state, int uniform, float lo, float hi, void* stream);
/* Direct kernel for the 3-channel image-producing layer: U[n,Cu,2h,2w] (NCHW) = act(convT(V) + b), Cu <= 4,
 * reading the reference weight tensor directly (models/nn/svhn.py:58-60). */
int mvk_conv4s2_up_nchw_small(const float* V, const float* Wref, const float* bias, float* U, int n, int h,
                              int w, int Cu, int Cv, int act, void* stream);

/* MFMA kernels for the same layer when h*w is a multiple of 64 (<= 256), Cu <= 4 and Cv in {16,32,64}
 * (mvk_conv4s2_small_up_supported != 0): one workgroup per image computes the column matrix
 * V[pos,:] . W[:,(cu,kh,kw)] on the matrix cores and gathers the output pixels from LDS (no wasted MFMA columns).
 * The backward entry point fuses backward-data (dV = conv(dUpre) * v_act'(V)), backward-weight (dWref +=) and
 * the bias gradient (db +=, nullable) with dUpre = dU * u_act'(Uout) applied while loading; db_v (nullable) +=
 * the per-channel sums of dV, i.e. the bias gradient of the layer that produced V; ws is split-K style scratch
 * (>= 512 * (16*Cu*Cv + Cu + Cv) floats for full parallelism). */
/* Forward of the image-CONSUMING layer (svhn.py:13-15, the encoder's first Conv2d(Cu <= 4, Cv, 4, 2, 1) on the NCHW
 * network input): V[n,h,w,Cv] = act(conv(U[n,Cu,2h,2w]) + bias), Wdown = the packed [16 Cu][Cv] weight of
 * mvk_pack_conv4s2_weight.  Same support set as mvk_conv4s2_small_up_supported; mvk_conv4s2_down routes here. */
int mvk_conv4s2_small_down_fwd(const float* U, const float* Wdown, const float* bias, float* V, int n, int h, int w,
                               int Cu, int Cv, int act, void* stream);
/* ... from the reference weight layout Wref[Cv][Cu][4][4]: the encoder's first kernel does not wait for mvk_pack_weights */
int mvk_conv4s2_small_down_fwd_wref(const float* U, const float* Wref, const float* bias, float* V, int n, int h, int w,
                                    int Cu, int Cv, int act, void* stream);
int mvk_conv4s2_small_up_supported(int h, int w, int Cu, int Cv);
int mvk_conv4s2_small_up_fwd(const float* V, const float* Wref, const float* bias, float* U, int n, int h, int w,
                             int Cu, int Cv, int act, void* stream);
int mvk_conv4s2_small_up_bwd(const float* dU, const float* Uout, int u_act, const float* V, int v_act,
                             const float* Wref, float* dV, float* dWref, float* db, float* db_v, float* ws,
                             int64_t ws_floats, int n, int h, int w, int Cu, int Cv, void* stream);
/* The fused decoder tail (round 3, opt-in for the in-package Decoder_VAE_SVHN, models/nn/svhn.py:52-70): the image-producing
 * layer scores its output against the data by a Normal(scale) likelihood (models/base/base_utils.py:62-87, mopoe_model.py:192-199)
 * in its own epilogue — rows[n] = -log p(x | image) summed over the image (what mvk_recon_nll_fwd produces from the image),
 * dpre[n,Cu,2h,2w] = d rows / d pre-activation stored where the image would be; X: [xrows][Cu * 4 h w] targets, image i is scored
 * against X[i % xrows] (the K samples of a data point share it).  mvk_conv4s2_small_up_bwd_pre is the layer's backward for that
 * buffer: dpre * rowscale[n] (d loss / d rows; NULL = 1) replaces dU * u_act'(Uout), the image is not read.  3 of the 5 passes over
 * the [K B, 3, 32, 32] tensor disappear.  Only where mvk_conv4s2_small_up_nll_supported returns 1 (16x16x32 -> 3x32x32). */
int mvk_conv4s2_small_up_nll_supported(int h, int w, int Cu, int Cv);
int mvk_conv4s2_small_up_fwd_nll(const float* V, const float* Wref, const float* bias, const float* X, int xrows, float scale,
                                 float* dpre, float* rows, int n, int h, int w, int Cu, int Cv, int act, void* stream);
int mvk_conv4s2_small_up_bwd_pre(const float* dpre, const float* rowscale, const float* V, int v_act, const float* Wref,
                                 float* dV, float* dWref, float* db, float* db_v, float* ws, int64_t ws_floats, int n, int h,
                                 int w, int Cu, int Cv, void* stream);
/* ..._fwd_nll with the stored gradient pre-multiplied by grad_weight (the weight the rows enter the loss with: a backward pass
 * whose upstream row gradient is exactly that constant passes rowscale = NULL and reads no row gradient) */
int mvk_conv4s2_small_up_fwd_nll_w(const float* V, const float* Wref, const float* bias, const float* X, int xrows, float scale,
                                   float grad_weight, float* dpre, float* rows, int n, int h, int w, int Cu, int Cv, int act,
                                   void* stream);
/* The image-producing layer (plain and fused-tail form) on scaled fp16 pairs: v_amax = device scalar bounding max |V|, published by
 * the launch that produced V (amax protocol above); the weight scale is derived in the kernel.  3 MFMAs per product, the weights as
 * the A operand (one 16-byte column-matrix write per tile), the fast sigmoid.  Same reference layer (models/nn/svhn.py:59-60
 * ConvTranspose2d(32, 3, 4, 2, 1) + Sigmoid) and likelihood (models/base/base_utils.py:62-87) as the entry points above; only
 * where mvk_conv4s2_small_up_nll_supported returns 1. */
int mvk_conv4s2_small_up_fwd_s(const float* V, const float* Wref, const float* bias, float* U, int n, int h, int w, int Cu, int Cv,
                               int act, const float* v_amax, void* stream);
int mvk_conv4s2_small_up_fwd_nll_s(const float* V, const float* Wref, const float* bias, const float* X, int xrows, float scale,
                                   float grad_weight, float* dpre, float* rows, int n, int h, int w, int Cu, int Cv, int act,
                                   const float* v_amax, void* stream);
/* The image layer's backward on scaled fp16 pairs (round 5; same reference lines as mvk_conv4s2_small_up_bwd_pre:
 * models/nn/svhn.py:58-60 ConvTranspose2d(32, 3, 4, 2, 1) + Sigmoid under models/base/base_utils.py:62-87's log-probability).
 * _fwd_nll_sy = _fwd_nll_s that also publishes an upper bound of max |dpre| into *dpre_amax (atomic max; must hold 0 before the
 * launch; from the largest row sum: at most sqrt(Cu 4 h w) times the true maximum); _bwd_pre_s = _bwd_pre_y with the gradient
 * image scaled under dpre_amax x max |rowscale| and V under v_amax (dv_amax may be NULL). */
int mvk_conv4s2_small_up_fwd_nll_sy(const float* V, const float* Wref, const float* bias, const float* X, int xrows, float scale,
                                    float grad_weight, float* dpre, float* rows, int n, int h, int w, int Cu, int Cv, int act,
                                    const float* v_amax, float* dpre_amax, void* stream);
int mvk_conv4s2_small_up_bwd_pre_s(const float* dpre, const float* rowscale, const float* V, int v_act, const float* Wref,
                                   float* dV, float* dWref, float* db, float* db_v, float* ws, int64_t ws_floats, int n, int h,
                                   int w, int Cu, int Cv, const float* dpre_amax, const float* v_amax, float* dv_amax,
                                   void* stream);

/* 1x1-spatial layers:
 *   unflatten  Y[n,(tap,co)] = act(z[n,Cin] Wp + b[co]), Wp[ci][tap*Cout+co] = Wref[ci][co][tap]
 *              (ConvTranspose2d(L,128,4,1,0), svhn.py:51) — forward / backward-data via mvk_gemm on Wp;
 *   flatten    Y[n,cv] = H[n,(tap,cu)] Wdown + b  (Conv2d(128,L,4,2,0) heads, svhn.py:29-30) — via mvk_gemm
 *              on the `down` packing.
 * The weight gradients scatter straight back into the reference layouts: */
int mvk_pack_unflatten_weight(const float* Wref, int Cin, int Cout, float* Wp, void* stream);
int mvk_unflatten_wgrad(const float* Z, const float* dY, float* dWref, int n, int Cin, int Cout, float* ws,
                        int64_t ws_floats, void* stream);
int mvk_flatten_wgrad(const float* H, const float* dY, float* dWref, int n, int Cu, int Cv, float* ws,
                      int64_t ws_floats, void* stream);

/* NCHW <-> NHWC copies at the plugin boundary. */
int mvk_nchw_to_nhwc(const float* src, float* dst, int n, int c, int h, int w, void* stream);
int mvk_nhwc_to_nchw(const float* src, float* dst, int n, int c, int h, int w, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The reference's public helper functions (multivae/models/base/base_utils.py) for user code that imports them
 * ------------------------------------------------------------------------------------------------ */
/* poe(mus, logvars, eps) (base_utils.py:122-130; stable = 0) and stable_poe (:133-147; stable = 1, no eps, an expert with
 * logvar = +inf has weight exactly 0, a single expert is returned as is): mus, lvs [E, n] -> mu, lv [n]; backward from
 * the gradients of both outputs (either may be NULL) to dmus, dlvs [E, n]. */
int mvk_poe_fwd(const float* mus, const float* lvs, int E, int64_t n, float eps, int stable, float* mu, float* lv,
                void* stream);
int mvk_poe_bwd(const float* mus, const float* lvs, int E, int64_t n, float eps, int stable, const float* gmu,
                const float* glv, float* dmus, float* dlvs, void* stream);
/* kl_divergence(mean, log_var, prior_mean, prior_log_var).sum(-1) (base_utils.py:90-119): kl [rows]; every operand holds
 * n_* elements and is indexed modulo that count (trailing-dimension broadcasting: a [1, L] prior under [rows, L]
 * posteriors).  Backward writes FULL-shape [rows, L] partial derivatives (NULL outputs are skipped); the caller column-
 * sums those of broadcast operands (mvk_colsum_acc). */
int mvk_kl_gauss_fwd(const float* mean, int64_t n_mean, const float* lv, int64_t n_lv, const float* pmean, int64_t n_pmean,
                     const float* plv, int64_t n_plv, int64_t rows, int L, float* kl, void* stream);
int mvk_kl_gauss_bwd(const float* mean, int64_t n_mean, const float* lv, int64_t n_lv, const float* pmean, int64_t n_pmean,
                     const float* plv, int64_t n_plv, int64_t rows, int L, const float* g, float* dmean, float* dlv,
                     float* dpmean, float* dplv, void* stream);
/* set_decoder_dist(dist, params)(recon, target) (base_utils.py:62-87) and cross_entropy (:28-57): ELEMENT-WISE log-
 * probabilities lp [n] of recon [n] against target [n_target] (indexed modulo n_target: a [B, D] target under [K, B, D]
 * reconstructions); dist = MVK_DIST_*; scale for normal / laplace; categorical: x * log_softmax(recon + eps) over the last
 * dimension C.  Backward: drecon = g * d lp / d recon. */
int mvk_logprob_fwd(const float* recon, const float* target, int64_t n, int64_t n_target, int dist, float scale, int C,
                    float eps, float* lp, void* stream);
int mvk_logprob_bwd(const float* recon, const float* target, int64_t n, int64_t n_target, int dist, float scale, int C,
                    float eps, const float* g, float* drecon, void* stream);

/* Up to MVK_COPY_MAX device-to-device copies in one launch (dst, src 16-byte aligned, bytes a multiple of 16): the tensors of one
 * collated batch (trainers/base/base_trainer.py:682-700: `inputs = set_inputs_to_device(inputs, device)`) into the input buffers a
 * replayed step reads.  Host array of descriptors, copied into the launch. */
#define MVK_COPY_MAX 8
typedef struct {
  void* dst;
  const void* src;
  int64_t bytes;
} mvk_copy_desc;
int mvk_copy_batch(const mvk_copy_desc* descs, int n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Optimizer
 * ------------------------------------------------------------------------------------------------ */
/* torch.optim.Adam (amsgrad=False) on flat buffers; step is 1-based; grad_scale multiplies g first
 * (1/world_size for DDP averaging).  trainers/base/base_trainer_config.py:58,62; base_trainer.py:350-361. */
int mvk_adam_step(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2,
                  double eps, double weight_decay, int step, double grad_scale, void* stream);
/* torch.optim.Adam(amsgrad=True) (the reference's MMVAE+ PolyMNIST setting, examples/mmvae_plus/mmnist.py:61-62): vmax is
 * the running maximum of exp_avg_sq (`max_exp_avg_sq`), updated in place and used in the denominator; vmax == NULL is
 * mvk_adam_step.  lr is a host scalar per call, so learning-rate schedulers (base_trainer_config.py:60) cost nothing. */
int mvk_adam_step_amsgrad(float* p, const float* g, float* m, float* v, float* vmax, int64_t n, double lr, double beta1,
                          double beta2, double eps, double weight_decay, int step, double grad_scale, void* stream);
/* The same update (vmax = NULL: plain Adam) that also CLEARS the gradient buffer as it consumes it when zero_grad != 0: the next
 * step's `optimizer.zero_grad()` (base_trainer.py:350) needs no pass over the buffer and no launch. */
int mvk_adam_step_fused(float* p, float* g, float* m, float* v, float* vmax, int64_t n, double lr, double beta1,
                        double beta2, double eps, double weight_decay, int step, double grad_scale, int zero_grad,
                        void* stream);
/* The optimizer inside a replayed hipGraph: the scalars of the update live in DEVICE memory.
 *   state    8 doubles owned by the caller: lr, beta1, beta2, eps, weight_decay, grad_scale, step (updates applied so far), 0
 *   scalars  8 floats (16-byte aligned) written by mvk_adam_prepare and read by mvk_adam_step_dev
 * mvk_adam_prepare (one thread) advances state[6] by one and derives the bias-corrected step size etc. in double, exactly the
 * arithmetic mvk_adam_step_fused does on the host; mvk_adam_step_dev is mvk_adam_step_fused with those scalars (buffers
 * 16-byte aligned, n % 4 == 0: the flat buffers of trainers.FlatParams).  Captured once, replayed every step: a learning-rate
 * scheduler (base_trainer_config.py:60) writes state[0] between replays; the pair is equivalent to one
 * optimizer.step() of base_trainer.py:350-361. */
int mvk_adam_prepare(double* state, float* scalars, void* stream);
int mvk_adam_step_dev(float* p, float* g, float* m, float* v, float* vmax, int64_t n, const float* scalars, int zero_grad,
                      void* stream);
/* The rotated step (trainers/graph.py: the decoder's late weight gradients of step N are produced at the head of step N + 1, beside
 * the encoders' forward pass).  optimizer.step() of base_trainer.py:350-361 is then TWO launches over disjoint ranges of the flat
 * buffers with the SAME scalars: mvk_adam_step_pub — mvk_adam_step_fused over the range whose gradients are final when the
 * step ends, which also leaves the update's scalars (step size, bias corrections, ...: 8 floats) in `publish` — and, inside the
 * next replay and behind the late gradients, mvk_adam_step_dev over the other range reading `publish`.  Every parameter is
 * updated exactly once per step and before it is next read.  n == 0 publishes only.  mvk_adam_identity writes the scalars
 * under which mvk_adam_step_dev changes nothing (the state before the first step and after a drain). */
int mvk_adam_step_pub(float* p, float* g, float* m, float* v, float* vmax, int64_t n, double lr, double beta1, double beta2,
                      double eps, double weight_decay, int step, double grad_scale, int zero_grad, float* publish, void* stream);
int mvk_adam_identity(float* scalars, void* stream);

/* The encoder heads in ONE launch: Y_h[m][n] = sum_k X[m][k] W_h(k, n) + b_h[n] for h = 0 (and 1 when W1 != NULL),
 * n < N <= 32, W_h(k, n) = W_h[k * w_sk + n * w_sn] (a torch Linear weight [N][K]: w_sk = 1, w_sn = K; the packed
 * Conv2d(C, L, 4, 2, 0) head [(kh,kw,c)][L]: w_sk = L, w_sn = 1).  Replaces `self.embedding(h)`, `self.log_var(h)` of
 * Encoder_VAE_MLP (models/nn/default_architectures.py:40-56) and `self.c1(e)`, `self.c2(e)` of Encoder_VAE_SVHN
 * (models/nn/svhn.py:29-34).  K % 4 == 0, X 16-byte aligned; exact fp32 (v_mfma_f32_16x16x4_f32), fixed summation
 * order.  b_h may be NULL. */
int mvk_heads_fwd(const float* X, const float* W0, const float* b0, float* Y0, const float* W1, const float* b1,
                  float* Y1, int M, int N, int K, int64_t w_sk, int64_t w_sn, void* stream);

/* Their backward in ONE launch (6 launches on the GEMM engine before: 2 weight gradients, 2 bias column sums, 2
 * backward-data products):  dX[m][k] = (sum_h sum_n dY_h[m][n] W_h(k, n)) * x_act'(X[m][k])  (x_act from the OUTPUT value
 * X; dX may be NULL),  dW_h += dY_h^T X  stored at dW_h[n * K + k], or at dW_h[n * K + (k % flat_c) * (K / flat_c) +
 * k / flat_c] when flat_c > 0 (k = (tap, c) of an NHWC map -> the [L][C][4][4] layout of the Conv2d heads),
 * db_h += column sums of dY_h (may be NULL),  dbprev += column sums of dX (may be NULL: the bias gradient of the layer that
 * produced X; K entries, or flat_c channel sums when flat_c > 0).  Per 128-row group a workgroup writes partial sums to slabs (the deferred arena of mvk_defer_begin when the
 * target lies in the flat gradient buffer, else `ws`: (2 N K + 2 N + K) * ceil(M / 128) floats at most); the groups are
 * added in order: deterministic.  N <= 32, K % 16 == 0, X / dX 16-byte aligned. */
int mvk_heads_bwd(const float* X, int x_act, const float* dY0, const float* dY1, const float* W0, const float* W1,
                  int64_t w_sk, int64_t w_sn, int flat_c, float* dX, float* dW0, float* dW1, float* db0, float* db1,
                  float* dbprev, int M, int N, int K, float* ws, int64_t ws_floats, void* stream);

/* Deferred leaf reductions.  Parameter gradients are leaves of the backward pass (reference: autograd accumulates them
 * into `.grad`, nothing reads them before `optimizer.step()`, trainers/base/base_trainer.py:405-420), so the ordered
 * finishes that complete them - split-K slabs of the weight-gradient GEMMs, per-workgroup column sums of the bias
 * gradients, the slabs of the convolution weight-gradient kernels - need not run one launch each behind their producer.
 * Between mvk_defer_begin and mvk_defer_end every entry point whose result ACCUMULATES into [grad, grad + grad_floats)
 * (the flat gradient buffer of trainers.FlatParams) writes its partial results into a private region of `arena` instead
 * of the caller's shared scratch and queues the finish; mvk_defer_flush(stream) orders `stream` behind every stream such a
 * producer ran on and runs all queued finishes in ONE launch per 24 (same fixed summation order per element as the
 * immediate kernels: results are bit-reproducible run to run).  A producer that does not fit (arena full, a second
 * accumulation into the same parameter while one is queued, a target outside the gradient buffer) finishes immediately
 * as without deferral.  The caller must flush before anything reads the gradient buffer (all-reduce, optimizer step) and
 * must keep `arena` alive and unused by others until then.  mvk_defer_flush may be called on ANY stream in the middle of
 * the backward pass (e.g. a side stream, once the decoders are done: the finishes then run beside the latency-bound
 * encoder backward); the arena regions it reads stay reserved and the next flush waits for it.  mvk_defer_end(stream) =
 * final flush on `stream` + off: after it (in stream order) the gradient buffer is complete.  mvk_defer_begin returns
 * MVK_EINVAL while finishes are pending; mvk_defer_pending = number of queued finishes. */
int mvk_defer_begin(float* arena, int64_t arena_floats, const float* grad, int64_t grad_floats);
int mvk_defer_flush(void* stream);
int mvk_defer_end(void* stream);
/* Arena floats asked for since the last mvk_defer_begin, granted or declined for lack of room: the host sizes the arena
 * from it (multivae_amd/kernels.py grows its arena between steps instead of reserving a fixed 512 MB). */
int64_t mvk_defer_wanted(void);
int mvk_defer_pending(void);

/* The collective of the data-parallel step (`allreduce_avg`; reference: the DDP wrapper of
 * trainers/base/base_trainer.py:92-117 averages the gradients over the ranks, :350-361 then steps the optimizer).  One process
 * per GPU; RCCL over xGMI, resolved at run time (dlopen: single-GPU processes never load it).
 *   mvk_comm_unique_id   rank 0 makes a rendezvous id of mvk_comm_id_bytes() bytes and hands it to every rank (any channel)
 *   mvk_comm_init        collective: every rank, same id, called with its own device current
 *   mvk_allreduce_avg    buf[i] <- mean over ranks, in place, enqueued on `stream` (no host synchronisation); nseg > 1 issues
 *                        nseg equal segments as one RCCL group
 *   mvk_comm_destroy */
int mvk_comm_id_bytes(void);
int mvk_comm_unique_id(void* id);
int mvk_comm_init(void** comm, int world, int rank, const void* id);
int mvk_comm_destroy(void* comm);
int mvk_allreduce_avg(float* buf, int64_t n, int nseg, void* comm, void* stream);
/* 1 when RCCL resolves in this process (no collective, no device work): ranks agree on the RCCL path BEFORE mvk_comm_init */
int mvk_comm_available(void);
/* world size and rank as the COMMUNICATOR reports them (ncclCommCount / ncclCommUserRank); either output may be NULL */
int mvk_comm_size(void* comm, int* world, int* rank);
/* The mean over the ranks of `nrange` disjoint ranges of one buffer (off / cnt: HOST arrays, in floats) as ONE RCCL group on
 * `stream`; a range longer than seg_floats (> 0) is cut into segments.  The overlapped data-parallel step issues the ranges
 * whose gradients are final early on a communication stream, behind an event of the replayed graph (mvk_event_record), and
 * the remaining ranges behind the end of the backward pass — DDP's bucket overlap (base_trainer.py:116-117,359) with two
 * buckets whose boundary is where the captured step says it is. */
int mvk_allreduce_avg_ranges(float* buf, const int64_t* off, const int64_t* cnt, int nrange, int64_t seg_floats, void* comm,
                             void* stream);
/* Events that cross the boundary of a replayed hipGraph: mvk_event_record(ev, external = 1, stream) on a CAPTURING stream adds
 * an event-record NODE (hipEventRecordWithFlags + hipEventRecordExternal), so a stream outside the graph can wait for a point
 * inside every replay (mvk_stream_wait_event, issued after the replay was launched).  external = 0 / a non-capturing stream:
 * a plain hipEventRecord. */
int mvk_event_create(void** ev);
int mvk_event_destroy(void* ev);
int mvk_event_record(void* ev, int external, void* stream);
int mvk_stream_wait_event(void* stream, void* ev);

/* Dense layers on pre-split fp16 pair planes (csrc/dense16.hip): the MLP decoder of the MnistSvhn models at the decoder batch
 * (reference: models/nn/default_architectures.py:225-258 Decoder_AE_MLP; likelihood models/base/base_utils.py:62-87).
 * A "planes" tensor [R][C] is two fp16 arrays hi, lo [R][C] with x s = hi + lo / 2048 (csrc/bf3.hpp); s is a power of two
 * derived from a device scalar `bound` >= max |x| (activations, gradients: one per tensor) or kept per plane ROW as inv[r] = 1 / s_r
 * (weights).  Every operand is split ONCE by its producer; the GEMM kernels move 16-byte pieces and issue three fp16 MFMAs per
 * fp32 product with no conversion arithmetic in the loop.  C % 8 == 0, 16-byte aligned planes.
 *   mvk_dense16_pack      W [N][K] (nn.Linear) -> planes [N][K] + nk_inv[N] (forward operand) and planes [K][N] + kn_inv[K]
 *                         (backward-data operand), one launch per step
 *   mvk_dense16_first     H planes [M][N] = act(Z [M][K] W^T + bias), K <= 32, N <= 1024 with 256 % (N / 4) == 0; *bound receives
 *                         the a-priori bound max_n ||W[n]||_1 z_amax + max |bias| the planes are scaled by (z_amax: device scalar
 *                         >= max |Z|, e.g. from mvk_amax)
 *   mvk_dense16_fwd_nll   the output layer + its likelihood: r = sigmoid(H W^T + bias) scored against X[m % xrows] by Normal(scale);
 *                         rows_part [mvk_dense16_fwd_nll_rows(N)][M] receives partial NLL row sums (their sum over the first axis
 *                         is -log p(x | r) of the row), G planes [M][N] = grad_weight * d NLL / d pre-activation under the bound
 *                         grad_weight (1 + x_amax) / (4 scale^2) written to *g_bound, colsum_part [mvk_dense16_colsum_rows(M)][N]
 *                         (optional) the column sums of G per row tile (the bias gradient's partials).  Neither the reconstruction
 *                         nor its gradient is written as an fp32 tensor.
 *   mvk_dense16_bwd_data  dA [M][N] fp32 = (G [M][K] planes x W planes [N][K] (the [K][N]-orientation pack of the layer's weight))
 *                         * ReLU'(mask) with mask_hi = the hi plane of the activation dA lands in (or NULL); db (optional) +=
 *                         column sums of dA (deferred finish when db lies in the registered gradient buffer, else ws)
 *   mvk_dense16_wgrad     dW [N][K] += G^T H over the M rows (both planes tensors; ordered finish of per-slice slabs: deferred,
 *                         else ws of >= slices * N * K floats), db [N] += the rows of colsum_part in order
 *   mvk_dense16_unsplit   planes -> fp32, optionally times rowf[m] * rowf_scale — rowf_tile > 0: rowf[(n / rowf_tile) M + m], one factor
 *                         per column tile and row, the layout of rows_part — (tests; the general backward when the upstream
 *                         row gradient is not the weight folded into G) */
int mvk_dense16_ok(int M, int N, int K);
int mvk_dense16_pack(const float* W, int N, int K, void* nk_hi, void* nk_lo, float* nk_inv, void* kn_hi, void* kn_lo,
                     float* kn_inv, void* stream);
int mvk_dense16_first(const float* Z, const float* W, const float* bias, const float* z_amax, void* hi, void* lo, float* bound,
                      int M, int N, int K, int act, void* stream);
int mvk_dense16_fwd_nll_rows(int N);
int mvk_dense16_colsum_rows(int M);
int mvk_dense16_fwd_nll(const void* h_hi, const void* h_lo, const float* h_bound, const void* w_hi, const void* w_lo,
                        const float* w_inv, const float* bias, const float* X, int xrows, const float* x_amax, float scale,
                        float grad_weight, void* g_hi, void* g_lo, float* g_bound, float* rows_part, float* colsum_part, int M,
                        int N, int K, void* stream);
int mvk_dense16_bwd_data(const void* g_hi, const void* g_lo, const float* g_bound, const void* wt_hi, const void* wt_lo,
                         const float* wt_inv, const void* mask_hi, float* dA, float* db, float* ws, int64_t ws_floats, int M, int N,
                         int K, void* stream);
int mvk_dense16_wgrad(const void* g_hi, const void* g_lo, const float* g_bound, const void* h_hi, const void* h_lo,
                      const float* h_bound, const float* colsum_part, int cs_rows, float* dW, float* db, float* ws,
                      int64_t ws_floats, int M, int N, int K, void* stream);
int mvk_dense16_unsplit(const void* hi, const void* lo, const float* bound, const float* rowf, float rowf_scale, int rowf_tile,
                        int M, int N, float* out, void* stream);
void mvk_dense16_debug(int flags); /* ablation switches of tools/dense16_probe.py (0 = the shipped kernels) */
void mvk_dense16_debug_stamps(float* four_floats); /* flag 16: where the forward kernel's cycle stamps go (NULL: nowhere) */

/* Nexus (models/nexus; nexus_model.py:209-254): the mean of the M <= MVK_MAX_MODALITIES message tensors msgs[m] [B, D] (HOST
 * array of device pointers) over the kept modalities of each row -> agg [B, D] (0 for a row with nothing kept) and keep_out [B, M]
 * (1 kept, 0 dropped or missing).  The keep set is, in this order of precedence: keep_in [B, M] (nonzero = kept), masks (HOST array
 * of M [B] availability vectors), or forced perceptual dropout drawn from u [B, M + 1] uniforms on [0, 1) (mvk_device_rng): the row is
 * dropped when u[b,0] < dropout_rate, then keeps 1 + floor(u[b,1] (M - 1)) modalities, the first ones of a partial Fisher-Yates
 * shuffle driven by u[b,2..]; all three NULL keeps everything.  bwd: dmsgs[m] [B, D] (HOST array, overwritten) =
 * keep[b,m] / count[b] * g[b]. */
int mvk_nexus_aggregate_fwd(const float* const* msgs, const uint8_t* const* masks, const float* keep_in, const float* u,
                            float dropout_rate, int M, int B, int D, float* agg, float* keep_out, void* stream);
int mvk_nexus_aggregate_bwd(const float* keep, const float* g, int M, int B, int D, float* const* dmsgs, void* stream);

/* Nexus top-level likelihood (nexus_model.py:153-168) for M modalities in one launch pair: rows[m][b] = gamma[m] mask_m[b]
 * sum_d -ln N(z_m[b,d] | r_m[b,d], s_m), s_m^2 = s2[m] = mean over the whole [B, D_m] block of (z_m - r_m)^2 when adapt[m],
 * else 1.  z, r, rows, masks (nullable), grows (entries nullable), dr: HOST arrays of device pointers; D, gamma, adapt: HOST
 * arrays.  q [M, B] (out: the row sums of (z - r)^2) and s2 [M] are kept for the backward pass; work: scratch of
 * M * ((B + 3) / 4) floats.  bwd: dr[m] [B, D_m] (overwritten) = d sum_b grows[m][b] rows[m][b] / d r_m, the path through s_m
 * included; z gets no gradient (it is detached).  Block sums are fixed-order two-stage reductions: deterministic.  masks[m] == NULL
 * inside a given array means modality m is complete; grows[m] == NULL means a zero gradient (dr[m] = 0).  An adapted modality whose
 * s2[m] comes out 0 (z_m == r_m, or differences so small that their squares underflow) is not special-cased: ln 0 and 1 / 0 give
 * what the float32 formulas give, rows[m] and dr[m] all NaN (masked rows included), s2[m] = 0; the other modalities are not
 * affected. */
int mvk_nexus_top_nll_fwd(const float* const* z, const float* const* r, const uint8_t* const* masks, const int* D,
                          const float* gamma, const int* adapt, int M, int B, float* const* rows, float* q, float* s2,
                          float* work, void* stream);
int mvk_nexus_top_nll_bwd(const float* const* z, const float* const* r, const uint8_t* const* masks, const int* D,
                          const float* gamma, const int* adapt, int M, int B, const float* const* grows, const float* q,
                          const float* s2, float* work, float* const* dr, void* stream);

/* Gaussian-mixture sampler: full-covariance EM on the device.  Replaces samplers/gaussian_mixture/gaussian_mixture_sampler.py:90-112
 * (sklearn.mixture.GaussianMixture(covariance_type="full").fit on the host copy of the embeddings) and :148-164 (gmm.sample);
 * the arithmetic is scikit-learn's _estimate_log_gaussian_prob, _estimate_gaussian_parameters,
 * _estimate_gaussian_covariances_full, _compute_precision_cholesky and the loop of BaseMixture.fit.  Per-row arithmetic is fp32,
 * every sum over rows and the per-component finish (regularisation, Cholesky, triangular inverse, log-determinant) are fp64,
 * outputs are fp32.  Bit-reproducible: per-workgroup partials go to `scratch` (mvk_gmm_scratch_bytes(L, C) bytes, independent of
 * N, 8-byte aligned) and are added in workgroup order.  1 <= L <= 64, 1 <= C <= 64 (else MVK_EINVAL); N = 0 is MVK_OK and writes
 * nothing.
 *   X [N,L] rows; weights [C]; means [C,L]; covs [C,L,L]; cov_chol [C,L,L] = the lower Cholesky factor of covs; prec_chol [C,L,L] =
 *   P_c = (cov_chol_c^-1)^T, upper triangular (scikit-learn's precisions_cholesky_); logdet [C] = sum ln diag P_c; resp [N,C].
 * mvk_gmm_estep, soft (hard = 0): resp = exp(log p(x_n, c) - lse_n), log p(x_n, c) = -1/2 (L ln 2 pi + |(x_n - mu_c) P_c|^2) +
 *   logdet[c] + ln w_c; row_out [N] (nullable) = lse_n; lb (nullable, DEVICE double) = mean_n lse_n.  Hard (hard = 1: identity
 *   precisions, equal weights; weights, prec_chol, logdet and lb are ignored): resp = one-hot of argmin_c |x_n - mu_c|^2 (first
 *   minimum), row_out = that minimum, labels [N] int32 (nullable) in / out, changed (nullable, device int32) = number of rows
 *   whose label changed: k-means (Lloyd) is this and mvk_gmm_mstep with means_only, k-means++ seeding reads row_out.
 * mvk_gmm_mstep: n_c = sum_n resp[n,c] + 10 FLT_EPSILON, means = sum resp x / n_c, covs = sum resp (x - mu_c)(x - mu_c)^T / n_c +
 *   reg_covar I centred on the NEW means (a second pass over the rows), weights = n_c / sum_c n_c, then cov_chol, prec_chol,
 *   logdet; a pivot that is not > 0 fills that component's cov_chol, prec_chol and logdet with NaN.  means_only: only means.
 * mvk_gmm_em_step: one iteration of BaseMixture.fit: E, M, then on `state` (DEVICE, 8 doubles, MVK_GMM_STATE_*; the caller sets
 *   LB = -inf and everything else 0 before the first step): PREV = LB, LB = the E-step's lower bound, ITER += 1, CONVERGED =
 *   |LB - PREV| < tol.  STATUS becomes 1 when a Cholesky pivot is not > 0 and 2 when the lower bound is not finite.  A step
 *   enqueued when CONVERGED or STATUS is non-zero changes nothing, so the host may enqueue several steps and read the block once.
 * mvk_gmm_sample: z[i] = means[comp[i]] + cov_chol[comp[i]] eps[i]; comp [n] int32, eps and z [n,L] (a component index outside
 *   [0, C) gives a NaN row). */
#define MVK_GMM_STATE_ITER 0
#define MVK_GMM_STATE_PREV 1
#define MVK_GMM_STATE_LB 2
#define MVK_GMM_STATE_CONVERGED 3
#define MVK_GMM_STATE_STATUS 4
#define MVK_GMM_STATE_PENDING 5 /* the lower bound of the step in flight */
#define MVK_GMM_STATE_DOUBLES 8
int mvk_gmm_scratch_bytes(int L, int C, int64_t* bytes);
int mvk_gmm_estep(const float* X, int64_t N, int L, int C, const float* weights, const float* means, const float* prec_chol,
                  const float* logdet, int hard, float* resp, float* row_out, int32_t* labels, int32_t* changed, double* lb,
                  void* scratch, void* stream);
int mvk_gmm_mstep(const float* X, const float* resp, int64_t N, int L, int C, double reg_covar, int means_only, float* weights,
                  float* means, float* covs, float* cov_chol, float* prec_chol, float* logdet, void* scratch, void* stream);
int mvk_gmm_em_step(const float* X, int64_t N, int L, int C, double reg_covar, double tol, float* weights, float* means,
                    float* covs, float* cov_chol, float* prec_chol, float* logdet, float* resp, double* state, void* scratch,
                    void* stream);
int mvk_gmm_sample(const float* means, const float* cov_chol, const int32_t* comp, const float* eps, int64_t n, int L, int C,
                   float* z, void* stream);

/* Batched k-means for the Clustering evaluator (multivae/metrics/latent_clustering/clustering_class.py:54-110 fits scikit-learn's
 * KMeans on a host copy of the training embeddings once per run, votes a class per cluster and classifies the test embeddings on
 * the host).  R independent fits of K centres on the SAME rows advance together: X [N,L] rows, centers [R,K,L], labels [R,N] int32,
 * all caller-owned.  The squared distance of a row is fp32 and direct (d = x - c, fmaf(d, d, .) in index order, never
 * |x|^2 - 2 x.c + |c|^2), the label is its first minimum; every sum over rows is fp64 from the first addend on, in a fixed order
 * (per thread, per workgroup, across workgroups through `scratch`: mvk_kmeans_scratch_bytes(L, K, R) bytes, independent of N,
 * 8-byte aligned); counts are integers (integer atomics); there is no floating-point atomic.  Bit-reproducible, and the bits of
 * run r do not depend on R.  1 <= L <= 64, 1 <= K <= 64, 1 <= R <= 32 (else MVK_EINVAL); N = 0 is MVK_OK and writes nothing; K > N
 * is legal.
 * mvk_kmeans_assign: labels (nullable) = argmin_k |x_n - c_rk|^2, d2 [R,N] (nullable) = that minimum, inertia [R] (nullable, DEVICE
 *   doubles, needs scratch) = its fp64 sum over the rows.  With y [N] int32 and table [R,K,n_classes+1] int64: table[r, label, y]
 *   += 1, a y outside [0, n_classes) counted in the extra last column (ACCUMULATED: the caller zeroes it; 1 <= n_classes <= 2^24).
 *   With y, majority [R,K] int32 and correct [R] int64: correct[r] += rows with majority[r, label] == y (ACCUMULATED).  One call
 *   serves the k-means++ distances, the final relabelling, the training contingency table and the test scoring.
 * mvk_kmeans_step: one iteration of scikit-learn's _kmeans_single_lloyd for every run whose CONVERGED is 0: labels from the current
 *   centres, new centre of a cluster = its fp64 row sum / its count stored as fp32, the centres are replaced, then on the run's block
 *   of `state` (DEVICE, [R, MVK_KMEANS_STATE_DOUBLES] doubles; the caller zeroes it and sets labels to -1 before the first step):
 *   ITER += 1, CHANGED = rows whose label changed, INERTIA = sum of the row minima (w.r.t. the centres the labels were taken from),
 *   SHIFT = sum (new - old)^2 over the stored centres, EMPTY += clusters without a row, CONVERGED = 1 when CHANGED is 0 (strict),
 *   else 2 when SHIFT <= *tol (tol: DEVICE double, so that the caller never synchronises to compute it).  A run whose CONVERGED
 *   is non-zero is untouched by further steps (centres, labels and state keep their bits), so the host may enqueue several steps
 *   and read the block once.  DEVIATION from scikit-learn: a cluster without rows keeps its previous centre and is counted in
 *   EMPTY; scikit-learn moves it to the row farthest from its own centre (a per-run top-k over the rows, for a path that
 *   well-seeded fits rarely take).
 * mvk_kmeans_vote: majority[r, k] = first maximum of table[r, k, 0 .. n_classes) (np.bincount(...).argmax(): ties go to the smallest
 *   class); a cluster with no row in a real class maps to its own index k (the reference's default entry of labels_dict). */
#define MVK_KMEANS_STATE_ITER 0
#define MVK_KMEANS_STATE_CONVERGED 1
#define MVK_KMEANS_STATE_SHIFT 2
#define MVK_KMEANS_STATE_CHANGED 3
#define MVK_KMEANS_STATE_INERTIA 4
#define MVK_KMEANS_STATE_EMPTY 5
#define MVK_KMEANS_STATE_DOUBLES 8
int mvk_kmeans_scratch_bytes(int L, int K, int R, int64_t* bytes);
int mvk_kmeans_assign(const float* X, int64_t N, int L, int K, int R, const float* centers, int32_t* labels, float* d2,
                      const int32_t* y, int n_classes, int64_t* table, const int32_t* majority, int64_t* correct, double* inertia,
                      void* scratch, void* stream);
int mvk_kmeans_step(const float* X, int64_t N, int L, int K, int R, const double* tol, float* centers, int32_t* labels,
                    double* state, void* scratch, void* stream);
int mvk_kmeans_vote(const int64_t* table, int R, int K, int n_classes, int32_t* majority, void* stream);

/* Image metrics of the evaluators (multivae/metrics/reconstruction/reconstruction.py: torchmetrics' StructuralSimilarityIndexMeasure
 * and a torch sum of squared differences).  preds, target [B,C,H,W] fp32, contiguous.  The SSIM of one update ("Metrics"):
 *   R = max(max preds - min preds, max target - min target) over the whole update, c1 = (0.01 R)^2, c2 = (0.03 R)^2;
 *   g[i] ~ exp(-((i - 5) / 1.5)^2 / 2), 11 taps normalised to sum 1, the 2-D weight is the outer product, per channel;
 *   only the (H - 10) x (W - 10) positions whose window lies inside the image; per position, with the weighted moments,
 *   ssim = (2 mu_p mu_t + c1) (2 s_pt + c2) / ((mu_p^2 + mu_t^2 + c1) (s_p^2 + s_t^2 + c2)), variances not clamped;
 *   ssim_rows[b] = the mean over the C (H - 10) (W - 10) positions of image b.  R = 0 gives NaN, and NaN propagates.
 * Arithmetic is fp32 with every variance and covariance centred on the local mean (no E[x^2] - mu^2); sums over positions, pixels
 * and rows are fp64 in a fixed order: two runs are bit-identical.
 * mvk_ssim_tile: the tile edge, in window positions, of the rows kernel (images of any H, W >= 11 are tiled).
 * mvk_ssim_scratch_bytes: the caller-owned scratch (8-byte aligned) of mvk_ssim_range and mvk_ssim_rows for that shape.
 * mvk_ssim_range: range[0] (DEVICE float) = R of the n elements of preds and of target; a NaN element gives NaN.  The scratch of
 *   any valid shape is large enough.
 * mvk_ssim_rows: ssim_rows [B] and sse_rows [B] (sse_rows[b] = sum over image b of (preds - target)^2).  R is read from range_dev
 *   (DEVICE float) unless that is NULL: then range_val is R.  mse_only != 0 writes sse_rows alone, reads neither range nor
 *   scratch nor ssim_rows (all may be NULL / 0), forms no window and takes any H, W >= 1: a [B, D] batch is C = H = 1, W = D.
 * mvk_ssim_accumulate: acc (DEVICE, MVK_SSIM_ACC_DOUBLES doubles) += {sum of ssim_rows, sum of sse_rows, B}, the rows added in
 *   index order in fp64; ssim_rows may be NULL (the SSIM sum is left alone).
 * MVK_EINVAL: a NULL pointer that is read or written, B or C <= 0, n <= 0, H or W < 11 (< 1 with mse_only), a grid of more than
 * 2^31 - 1 tiles. */
#define MVK_SSIM_ACC_SSIM 0
#define MVK_SSIM_ACC_SSE 1
#define MVK_SSIM_ACC_ROWS 2
#define MVK_SSIM_ACC_DOUBLES 3
int mvk_ssim_tile(void);
int mvk_ssim_scratch_bytes(int B, int C, int H, int W, int64_t* bytes);
int mvk_ssim_range(const float* preds, const float* target, int64_t n, float* range, void* scratch, void* stream);
int mvk_ssim_rows(const float* preds, const float* target, int B, int C, int H, int W, const float* range_dev, float range_val,
                  int mse_only, float* ssim_rows, float* sse_rows, void* scratch, void* stream);
int mvk_ssim_accumulate(const float* ssim_rows, const float* sse_rows, int B, double* acc, void* stream);

/* Frechet statistics for the FIDEvaluator (multivae/metrics/fids/fids.py:112-156 keeps every batch's activations in a list,
 * copies all of them to the host and takes np.mean and np.cov there).  Two feature streams of width D (stream 0 = real data X0,
 * stream 1 = generated data X1; [n, D] fp32 rows, contiguous) are folded batch by batch into a caller-owned `state` (DEVICE,
 * mvk_fd_state_bytes(D) bytes, 8-byte aligned) that holds per stream a shift c[D] (fp32), the row count (int64),
 * S1[D] = sum (x - c) and S2 = sum (x - c)(x - c)^T (fp64; only the mvk_fd_tile() x mvk_fd_tile() tiles on or above the diagonal
 * are computed and stored).  c is the column mean of the stream's FIRST batch and never changes: features far from zero lose
 * their covariance to cancellation in un-shifted fp32 raw moments.  Within a call x - c is fp32, the rows are walked in chunks of
 * mvk_fd_chunk() rows, the chunk's (X - c)^T (X - c) is formed with the f32-input MFMA (bit for bit a row-ordered fmaf chain) and
 * every chunk is added to fp64; S1 is fp64 from the first addend on.  A state element is written by exactly one workgroup per
 * launch and there is no floating-point atomic: the same sequence of calls gives the same bits.  Any D >= 1 up to 65535 tiles per
 * edge, any n >= 1.
 * mvk_fd_tile / mvk_fd_chunk: the tile edge of S2 and the rows per chunk (not statuses).
 * mvk_fd_state_bytes: the size of `state` for two streams.
 * mvk_fd_begin: zeroes the state and sets each stream's shift to the column mean of its n rows (rows added in row order in fp64,
 *   stored as fp32).  It adds no row: the caller follows it with mvk_fd_update on the same batch.  X1 may be NULL: stream 1 is
 *   left empty with a zero shift.
 * mvk_fd_update: adds the n rows of X0 to stream 0 and, unless X1 is NULL, the n rows of X1 to stream 1, in one launch.
 * mvk_fd_finish: mean [2,D] fp64 = c + S1 / n; cov [2,D,D] fp64 = (S2 - S1 S1^T / n) / (n - 1), the full matrix, the lower
 *   triangle mirrored bit for bit from the upper (np.cov(rowvar=False); n = 1 gives NaN as numpy does, an empty stream NaN);
 *   terms (MVK_FD_TERMS doubles) = {|mean0 - mean1|^2, tr cov0, tr cov1, n0, n1}.  The state is left as it was.
 * MVK_EINVAL: D < 1 or too large, n < 1, X0 or state NULL, a NULL output. */
#define MVK_FD_TERM_DMEAN2 0
#define MVK_FD_TERM_TRACE0 1
#define MVK_FD_TERM_TRACE1 2
#define MVK_FD_TERM_N0 3
#define MVK_FD_TERM_N1 4
#define MVK_FD_TERMS 5
int mvk_fd_tile(void);
int mvk_fd_chunk(void);
int mvk_fd_state_bytes(int D, int64_t* bytes);
int mvk_fd_begin(const float* X0, const float* X1, int64_t n, int D, void* state, void* stream);
int mvk_fd_update(const float* X0, const float* X1, int64_t n, int D, void* state, void* stream);
int mvk_fd_finish(void* state, int D, double* mean, double* cov, double* terms, void* stream);

/* PolyMNIST classifier (multivae/metrics/classifiers/mmnist.py, eval mode: dropout is the identity) with what the coherence
 * evaluator does with its logits, in one launch: x [n,3,28,28] fp32 contiguous -> conv 4x4 / stride 2 / padding 1 (10) + ReLU ->
 * conv 4x4 / stride 2 / padding 1 (20) + ReLU -> flatten in (c, h, w) order -> 980 -> 128 + ReLU -> 10.  The weights are the
 * module's parameters in PyTorch's layouts, read in place (no packed copy exists, so nothing has to be invalidated):
 * w1 [10,3,4,4], b1 [10], w2 [20,10,4,4], b2 [20], w3 [128,980], b3 [128], w4 [10,128], b4 [10].
 * Outputs, each may be NULL (not all three):
 *   logits [n,10] fp32;
 *   pred [n] int32 = torch.argmax(logits, 1): the first maximum, a NaN logit counting as the maximum;
 *   counts [11,2] int64, ACCUMULATED (ClassCounts.update): row i has the label labels[i % label_rows] (int64; the sample-major
 *   stacking of nb_samples_for_cross > 1 generations over label_rows data rows), r = the label, or 10 for a label outside
 *   [0, 10): counts[r][0] += (pred == label), counts[r][1] += 1.  Integer atomics; there is no floating-point atomic.
 * Every product and sum is fp32 (plain FMAs in the convolutions and fc2, the f32-input MFMA in fc1), each logit one fixed
 * sequence of operations on its own image: the logits of an image are bit-identical from run to run, for every n and wherever
 * the image falls among the mvk_polyclf_tile() images of a workgroup.  No activation goes to global memory.
 * mvk_polyclf_tile: images per workgroup (not a status).
 * n == 0 is MVK_OK and writes nothing.  MVK_EINVAL: n < 0; all three outputs NULL; counts without labels, or with
 * label_rows <= 0 or n % label_rows != 0; x or a weight NULL with n > 0. */
int mvk_polyclf_tile(void);
int mvk_polyclf_fwd(const float* x, int64_t n, const float* w1, const float* b1, const float* w2, const float* b2, const float* w3,
                    const float* b3, const float* w4, const float* b4, float* logits, int32_t* pred, const int64_t* labels,
                    int64_t label_rows, int64_t* counts, void* stream);

/* PolyMNIST convolutional networks (multivae/models/nn/mmnist.py:36-206): 3x3 / stride 2 / padding 1 convolutions on the map
 * chain 28 -> 14 -> 7 -> 4 and their transposes with output_padding 0 or 1 (csrc/polyconv.hip).  The big map U is [n,H,W,Cu]
 * (u_nchw != 0, Cu == 3 only: the image [n,3,H,W]), the small map V is [n,h,w,Cv] with h = (H + 1) / 2, w = (W + 1) / 2; H and
 * W are always those of the BIG map, which fixes output_padding.  Wref is the parameter in PyTorch's layout, read in place:
 * Conv2d(Cu, Cv, 3, 2, 1).weight and ConvTranspose2d(Cv, Cu, 3, 2, 1, output_padding).weight are both [Cv][Cu][3][3], and the
 * transposed layer is the adjoint of the strided one.  fp32 in and out on the exact f32-input MFMA; every entry is one fixed
 * sequence of operations on its own image (no floating-point atomics, ordered finishes): results are bit-identical from run to
 * run, and those of down / up and of the fused trunks do not depend on n or on the image's place in a tile.
 *   mvk_conv3s2_ok     1 where the entries below take the problem: (Cu, Cv) in {(3,32), (32,64), (64,128)}, 1 <= H, W <= 4096.
 *                      They return MVK_EINVAL where it returns 0.
 *   mvk_conv3s2_down   V = act(conv(U) + bias) (* v_act'(v_act_src), laid out like V): Conv2d forward, ConvTranspose2d
 *                      backward-data.  bias and v_act_src may be NULL.
 *   mvk_conv3s2_up     U = act(convT(V) + bias) (* u_act'(u_act_src), laid out like U): ConvTranspose2d forward, Conv2d
 *                      backward-data.  Output positions are walked by parity class (1, 2, 2 and 4 taps).
 *   mvk_conv3s2_wgrad  dWref[Cv][Cu][3][3] (+)= sum over positions of U(gathered) V (accumulate != 0: +=), and with db != NULL
 *                      db (+)= the per-channel sums of V (db_side 1, [Cv]: the Conv2d bias) or of U (db_side 2, [Cu]: the
 *                      ConvTranspose2d bias); db_side 0 with db NULL.  Position slices go to slabs in ws (at least
 *                      9 Cu Cv + 128 floats) and are added in a fixed order; slicing and order depend on the shape and ws_floats alone.
 *   mvk_polyenc_fwd    no-grad encoder trunk in one launch: x [n,3,28,28] -> 3 x (conv + bias + ReLU) -> h3 [n,4,4,128] (NHWC).
 *                      A workgroup owns mvk_polyconv_tile() images; the 14x14x32 and 7x7x64 maps stay in LDS.
 *   mvk_polydec_fwd    the decoder's mirror: h0 [n,4,4,128] (NHWC) -> convT + ReLU (7x7x64) -> convT + ReLU (14x14x32) -> convT
 *                      -> [n,3,28,28] (NCHW).  Weights w0 [128,64,3,3], w1 [64,32,3,3], w2 [32,3,3,3].
 * The fused trunks run the layer routine of down / up: their results equal the three layer launches bit for bit.
 * NHWC operands read four channels at a time must be 16-byte aligned (MVK_EINVAL otherwise); n == 0 is MVK_OK. */
int mvk_conv3s2_ok(int H, int W, int Cu, int Cv);
int mvk_polyconv_tile(void);
int mvk_conv3s2_down(const float* U, const float* Wref, const float* bias, float* V, int n, int H, int W, int Cu, int Cv, int act,
                     int u_nchw, const float* v_act_src, int v_act, void* stream);
int mvk_conv3s2_up(const float* V, const float* Wref, const float* bias, float* U, int n, int H, int W, int Cu, int Cv, int act,
                   int u_nchw, const float* u_act_src, int u_act, void* stream);
int mvk_conv3s2_wgrad(const float* U, const float* V, float* dWref, float* db, int db_side, int n, int H, int W, int Cu, int Cv,
                      int u_nchw, int accumulate, float* ws, int64_t ws_floats, void* stream);
int mvk_polyenc_fwd(const float* x, int64_t n, const float* w0, const float* b0, const float* w1, const float* b1, const float* w2,
                    const float* b2, float* h3, void* stream);
int mvk_polydec_fwd(const float* h0, int64_t n, const float* w0, const float* b0, const float* w1, const float* b1, const float* w2,
                    const float* b2, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * CUB text encoder (models/nn/cub.py CubTextEncoder): the stages of a post-norm transformer encoder over short sentences
 * that are not GEMMs (csrc/textenc.hip).  tokens [B,S] int64; activations [B,S,E] fp32; the packed in-projection
 * qkv [B,S,3E] (q | k | v, head h owning columns h*hd .. h*hd + hd - 1 of each third, hd = E / nhead).
 *
 * Dropout.  Every site reads uniform noise u in [0,1) from a caller-owned buffer: an element is kept iff u >= p and then
 * scaled by 1 / (1 - p); the backward entries re-read the same noise (no mask is stored).  noise == NULL or p == 0: no
 * dropout.  0 <= p < 1.  One forward's noise is ONE flat buffer, the sites in this order (floats):
 *   pos [B,S,E], then per layer: attn [B,nhead,S,S], res1 [B,S,E], ff [B,S,F], res2 [B,S,E];
 * every entry takes the pointer of its own site.
 *
 * Every sum runs in a fixed order and there is no floating-point atomic: results are bit-identical from run to run.
 * Optional pointers may be NULL.  MVK_EINVAL: a required pointer NULL, a size < 1, p outside [0,1), and what each entry
 * names. */
/* out[b,s,:] = drop(emb[tokens[b,s],:] * sqrt(E) + pe[s,:]); emb [V,E], pe [>= S,E].  A token outside [0,V) reads no
 * embedding row (its embedding counts as 0). */
int mvk_txt_embed_fwd(const int64_t* tokens, const float* emb, const float* pe, const float* noise, float p, float* out,
                      int B, int S, int E, int V, void* stream);
/* dE[v,:] (+= when accumulate != 0, else =) sqrt(E) * sum over (b,s) with tokens[b,s] == v of keep * scale * (g + g2)[b,s,:],
 * the rows that share a token added in (b,s) order; a row no token names gets 0 (accumulate == 0) or stays.  g2 (the
 * second gradient of the residual stream) may be NULL. */
int mvk_txt_embed_bwd(const int64_t* tokens, const float* g, const float* g2, const float* noise, float p, float* dE,
                      int accumulate, int B, int S, int E, int V, void* stream);
/* One workgroup per (sentence, head): scores = (q / sqrt(hd)) k^T, keys with keymask[b,j] == 0 at -inf (keymask int32
 * [B,S], NULL = every key real), P = softmax over j, ctx[b,i,h*hd + d] = sum_j drop(P)[i,j] v[j,d].  P [B,nhead,S,S]
 * receives the probabilities BEFORE dropout (NULL: not kept).  A sentence with no real key gives NaN, like torch.
 * 1 <= S <= MVK_TXT_MAX_SEQ, E % nhead == 0, hd <= MVK_TXT_MAX_HEAD_DIM. */
#define MVK_TXT_MAX_SEQ 64
#define MVK_TXT_MAX_HEAD_DIM 128
int mvk_txt_attn_fwd(const float* qkv, const int32_t* keymask, const float* noise, float p, float* P, float* ctx,
                     int B, int S, int E, int nhead, void* stream);
/* dqkv [B,S,3E] from dctx [B,S,E], with D = keep * scale of the attention site:  dV = (P o D)^T dctx,
 * dP = (dctx V^T) o D, dS = P o (dP - rowsum(dP o P)), dQ = dS K / sqrt(hd), dK = dS^T Q / sqrt(hd).  Same limits. */
int mvk_txt_attn_bwd(const float* qkv, const float* P, const float* dctx, const float* noise, float p, float* dqkv,
                     int B, int S, int E, int nhead, void* stream);
/* z = x + drop(t), y = (z - mean) * rstd * gamma + beta over the E entries of each of `rows` rows (biased variance,
 * rstd = 1 / sqrt(var + eps)).  gamma / beta NULL: 1 / 0.  z [rows,E] (may be NULL, may alias t), mean, rstd [rows] (may
 * be NULL) are what the backward reads.  zero_pads != 0 with rowmask (int32 [rows], 0 = padded): y = 0 on padded rows
 * (the last layer of an evaluation forward).  y must not alias x or t. */
int mvk_txt_add_ln_fwd(const float* x, const float* t, const float* noise, float p, const float* gamma, const float* beta,
                       float eps, const int32_t* rowmask, int zero_pads, float* y, float* z, float* mean, float* rstd,
                       int64_t rows, int E, void* stream);
/* With g = (dy + dy2) * gamma and xh = (z - mean) * rstd:  dx = rstd * (g - mean_e(g) - xh * mean_e(g * xh)) (the residual
 * stream), dt = keep * scale * dx (through the dropout; NULL: not wanted — without dropout dt == dx),
 * dgamma[e] += sum_r (dy + dy2) * xh, dbeta[e] += sum_r (dy + dy2): column sums in two stages, slabs of 64 rows into ws
 * (needs 2 * E * ceil(rows / 64) floats, MVK_EINVAL below that) and then over the slabs in order.  dy2, dt, dgamma, dbeta
 * may be NULL (ws too when both sums are). */
int mvk_txt_add_ln_bwd(const float* dy, const float* dy2, const float* z, const float* mean, const float* rstd,
                       const float* gamma, const float* noise, float p, float* dx, float* dt, float* dgamma, float* dbeta,
                       float* ws, int64_t ws_floats, int64_t rows, int E, void* stream);
/* x = keep * scale * x in place over n floats: the feed-forward dropout, forward (on relu(W1 h + b1)) and backward (on the
 * gradient of that product) alike. */
int mvk_txt_drop(float* x, const float* noise, float p, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The image grid of a set of modality tensors (metrics.Visualization, BaseTrainer.predict)
 * ------------------------------------------------------------------------------------------------ */
/* data/datasets/utils.py:50-91 (adapt_shape) -> torch.cat -> torchvision.utils.make_grid(nrow, padding, pad_value;
 * normalize=False) -> mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(uint8) (metrics/visualization/
 * visualization_class.py:93-108, trainers/base/base_trainer.py:830-917) in one launch that writes every element of its
 * outputs exactly once (no memset in front, no atomics).
 *   srcs   HOST array of S <= MVK_GRID_MAX_SOURCES descriptors, copied into the launch: `data` a device tensor
 *          [n, c, h, w] of contiguous fp32.  The tiles are the images of source 0, then of source 1, ...: T = sum n.
 *          A source with n == 0 adds no tile and does not count towards the tile size (its data may be NULL).
 *   channels  c == 1: replicated to three; c == 2: the third channel is 0; c >= 3: the first three.
 *   centring  H = max h, W = max w over the sources.  An image sits in its H x W tile behind floor((H - h) / 2) rows and
 *          floor((W - w) / 2) columns of zeros (the ceil of each follows it).  These zeros are part of the tile: 0,
 *          not pad_value.
 *   grid   xmaps = min(nrow, T), ymaps = ceil(T / xmaps), Hg = ymaps (H + padding) + padding, Wg = xmaps (W + padding)
 *          + padding; tile k has its corner at row (k / xmaps) (H + padding) + padding, column (k % xmaps) (W + padding)
 *          + padding; every other pixel, the empty cells of a last row included, is pad_value.  T == 1 is make_grid's
 *          exception: the single image without a border, Hg = H, Wg = W.
 * outputs (either may be NULL)
 *   grid   [3, Hg, Wg] fp32 (any 4-byte aligned address): copies of the inputs, bit for bit
 *   image  [Hg, Wg, 3] uint8 (any address): (uint8) clamp(fl(fl(255 x) + 0.5), 0, 255), the product rounded to fp32 before
 *          the sum is (never an fma); +inf gives 255, -inf 0, and a NaN gives 0.
 * MVK_EINVAL: S > MVK_GRID_MAX_SOURCES, nrow <= 0, padding < 0, a negative n, a non-positive c, h or w, 3 Hg Wg >= 2^31
 * (all decided from the descriptors' shapes, before `data` is looked at and before any launch), a NULL `data` of a
 * source with images.  T == 0 is a no-op that returns MVK_OK.  mvk_image_grid_size reports T, Hg and Wg (0, 0, 0 for
 * T == 0) under the same refusals and reads no `data`. */
#define MVK_GRID_MAX_SOURCES 32
typedef struct {
  const float* data;
  int32_t n, c, h, w;
} mvk_grid_src;
int mvk_image_grid_size(const mvk_grid_src* srcs, int S, int nrow, int padding, int64_t* T, int64_t* Hg, int64_t* Wg);
int mvk_image_grid(const mvk_grid_src* srcs, int S, int nrow, int padding, float pad_value, float* grid, uint8_t* image,
                   void* stream);

/* ------------------------------------------------------------------------------------------------
 * A batch of a device-resident dataset (data/datasets/cub.py, CUB.device_batcher)
 * ------------------------------------------------------------------------------------------------ */
/* The rows of a store picked by a device index tensor, expanded to what the models take; one launch each, on the caller's
 * stream, nothing synchronises.  Every output element is written exactly once (no memset in front, no atomics); the outputs
 * may begin at any 4-byte (out_tokens: 8-byte) aligned address.  The indices are taken ON TRUST: the caller checks
 * 0 <= index[b] < N (captions) and index[b] / div < N (images) on the host before it copies an epoch's order to the device.
 *
 * mvk_text_batch: the captions of a batch, with r = index[b]:
 *   out_tokens[b, l]   = tokens[r, l]                       int64 [B, L], or NULL
 *   padding_mask[b, l] = l < lengths[r] ? 1 : 0             fp32 [B, L]
 *   one_hot[b, l, c]   = c == tokens[r, l] ? 1 : 0          fp32 [B, L, V], or NULL (a token outside [0, V) gives a zero row)
 * mvk_u8_image_batch: the pictures of a batch from a byte store [N, E]:
 *   out[b, e] = float(store[index[b] / div, e]) / 255       fp32 [B, E]; the IEEE division, bit for bit torch's
 *                                                           .float().div(255); div = 10: the ten captions of a CUB picture
 * B == 0 returns MVK_OK without a launch.  MVK_EINVAL: a NULL required pointer, L < 1, V < 1, E < 1, div < 1, a negative
 * B or N, N == 0 with B > 0, a misaligned output. */
int mvk_text_batch(const int32_t* tokens, const int32_t* lengths, const int64_t* index, int64_t N, int B, int L, int V,
                   int64_t* out_tokens, float* padding_mask, float* one_hot, void* stream);
int mvk_u8_image_batch(const uint8_t* store, const int64_t* index, int64_t N, int B, int64_t E, int div, float* out,
                       void* stream);

/* Device-timestamp profiler (bench.py's roofline objects).  device_slots: nslots records of MVK_PROF_SLOT_U64 = 520
 * uint64 each: [0] sum of durations (clock ticks, first workgroup in -> last workgroup out), [1] launches accumulated,
 * [2] sum of (first workgroup in -> start of the one-wave fold kernel queued behind the launch: the launch has drained
 * its stores by then; this bracket contains what a kernel trace reports), [8 + 8 e] start stamps, [264 + 8 e] end stamps
 * (e < 32); the caller initialises the start stamps to ~0 and everything else to 0.  Every instrumented launch
 * (kind 1: fused reconstruction NLL forward, 2: imgconv up, 3: imgconv down, 4: imgconv weight gradient, 5 / 6: image-
 * layer forward / backward) takes the next record: its workgroups stamp the constant-rate clock on entry (min) and exit
 * (max), and a one-wave kernel behind it adds max(end) - min(start) to the sum and re-arms the record, so a launch
 * captured into a hipGraph accumulates one duration per replay.  host_kinds / host_work (nslots entries, may be NULL)
 * receive the kind and the algorithmic work of the launch (bytes for the HBM-bound kinds 1, 5, 6, FLOP for the
 * others).  device_slots == NULL switches the profiler off (later launches are not stamped; captured ones keep their
 * record). */
int mvk_prof_enable(void* device_slots, int nslots, int32_t* host_kinds, double* host_work);
int mvk_prof_count(void);     /* records taken since mvk_prof_enable */
/* n one-wave kernels back to back, each storing the clock at its first and last instruction into device_ticks[2 i],
 * device_ticks[2 i + 1] (uint64): first[i + 1] - last[i] is the dependent-kernel boundary that the retire bracket of a
 * record contains once. */
int mvk_prof_calibrate(void* device_ticks, int n, void* stream);
int mvk_prof_clock_khz(void); /* rate of the stamped clock */

/* Measurement hooks.  The phase buffer is read by a -DMVK_PHASES build of the library only (per-phase cycle counters of
 * the GEMM main loop accumulated into an 8-entry device buffer) and is inert in the shipped build.  The flags are host-side
 * dispatch bits in every build: 0x100 / 0x200 take the register-stationary 4x4 stride-2 kernels never / for every batch
 * size, 0x400 / 0x800 the same for the register-stationary 3x3 kernels. */
void mvk_debug_set_phase_buffer(unsigned long long* device_counters);
void mvk_debug_set_flags(int flags);

#ifdef __cplusplus
}
#endif
#endif /* MVK_H */
