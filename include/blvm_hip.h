/* blvm_hip.h — C ABI of libblvm_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for the blvm hot path.
 *
 * The reference (JakobHavtorn/benchmarking-lvms, package `blvm`) is pure Python on PyTorch and has NO FFI of its
 * own (`setup.py:57` ext_modules=[]); every entry point below replaces a chain of ATen ops at the cited reference
 * lines (paths relative to the reference checkout).  INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions
 *   - All tensors are device pointers to row-major fp32 unless stated; reductions that the reference carries in
 *     float64 (`blvm/models/vrnn.py:266`) are double.
 *   - The caller owns every buffer (inputs, outputs, workspace/reserve); the library never allocates, frees or
 *     retains a pointer past the call.
 *   - Apart from inputs, from buffers an entry point adds into (marked ACCUMULATED, "+=" or "caller zeroes")
 *     and from the ticket words of the fused DMoL backward's workspace (zero between launches), no result of
 *     any entry point depends on what its output, reserve, workspace or scratch buffers held before the call:
 *     they may be uninitialised.
 *   - All work is enqueued on the caller's `stream` (a hipStream_t passed as void*); no implicit device sync.
 *   - Return value: 0 on success, a negative BLVM_E* code otherwise; text via blvm_last_error() (thread-local).
 *   - Sequence tensors are TIME-MAJOR [T', B, F] (one contiguous slab per recurrent step).
 */
#ifndef BLVM_HIP_H
#define BLVM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BLVM_OK 0
#define BLVM_EINVAL (-1)  /* bad shape / alignment / null pointer */
#define BLVM_ELAUNCH (-2) /* HIP launch or runtime error */
#define BLVM_ENOSUP (-3)  /* configuration not supported by this build */
#define BLVM_NOT_APPLICABLE 1 /* not an error: the call did nothing because the shape is outside this entry point; take the general one */

int blvm_version(void);
const char* blvm_last_error(void);
/* 1 if a gfx950 device is visible to the HIP runtime, else 0 (never throws). */
int blvm_device_ok(void);
/* The recurrent sequences (K1-K5) run as ONE persistent launch whose workgroups wait for each other with BOUNDED spins.  A spin
 * that gives up (a workgroup of the launch was not resident: another process holds CUs) drains its launch with garbage results; the
 * call that enqueued it has long returned BLVM_OK.  This reports such launches: the number so far in this process (0 = none) and
 * the code (step << 4 | link) of the last spin that failed.  Reads pinned host memory; never blocks.  Check it where results are
 * read back (the reference's loops synchronise when they read the loss, `experiments/experiment_vrnn_audio.py:232`). */
int blvm_async_errors(unsigned* last_code);
/* The same counter with read-and-clear semantics: aborted launches since the previous take (and the code of the last one, 0 if
 * none).  For loops that handle an abort (drop the step, all-reduce the count over ranks so that every rank leaves together) and go
 * on: the sticky total above would fail every later check of the process. */
int blvm_async_errors_take(unsigned* last_code);
/* Execution switch of K1-K5 (results agree to fp32 summation order): sequences with at most `max_batch` rows run as one
 * persistent launch, larger ones as one launch per link (0 = always per link; < 0 = leave unchanged; default 128 or env
 * BLVM_PCHAIN_MAX_B / BLVM_PCHAIN=0; the VRNN pair also runs batches of 65 .. 256 rows persistently, on 32-row tiles).  The
 * persistent kernels run 16 waves per workgroup: `waves` <= 0 or 16 leaves that as it is, any other value is BLVM_EINVAL. */
int blvm_pchain_configure(int max_batch, int waves);
int blvm_pchain_max_batch(void); /* the current limit (at most 128) */
/* Operand type of the matrix products — the reference's `--use_amp True` switch (`experiments/experiment_vrnn_audio.py:198,219-230`:
 * torch.autocast around forward).  BLVM_DTYPE_F32 (default): fp32 operands, exact fp32 fma chains.  BLVM_DTYPE_BF16: the
 * persistent recurrent chains (K1-K5 with B <= blvm_pchain_max_batch()) and the K6 GEMMs round their operands to bf16 (nearest
 * even) and multiply on the bf16 matrix pipe; accumulation, epilogues, reductions, likelihoods and everything stored stay fp32
 * (autocast keeps bf16 outputs; this mode is at least as precise).  BLVM_DTYPE_F16: the same products with operands rounded to
 * fp16 (nearest even, |x| >= 65520 -> inf, exactly torch's .half()) on the fp16 matrix pipe — the type the reference's autocast
 * uses; its gradients need loss scaling (torch.amp.GradScaler), as the reference's do.  Paths that decline the 16-bit modes (row
 * groups, launch per link, static walks, conv coders) run fp32 in both.  Also settable with env BLVM_DTYPE=bf16 / f16 before the
 * first call. */
#define BLVM_DTYPE_F32 0
#define BLVM_DTYPE_BF16 1
#define BLVM_DTYPE_F16 2
int blvm_set_operand_dtype(int dtype);
int blvm_get_operand_dtype(void);
/* Diagnostics: while `device_buffer` (64 zero-initialised uint64 in device memory, caller-owned) is installed, the persistent kernels
 * add the 100 MHz wall-clock ticks two of their workgroups spend in every descriptor of the step program (waits included): words
 * [0..31] workgroup 0 (critical path), [32..55] the first workgroup of the deferred range ([64..127]: the same for backward
 * programs; pass 128 words).  NULL uninstalls. */
int blvm_pchain_profile(unsigned long long* device_buffer);
/* Diagnostics: placement bits of the persistent programs (results unchanged; default 84 = 4 | 16 | 64): 4 XCD-aware column-tile placement (a
 * column tile's row tiles on one XCD, so every XCD's L2 holds 1/8 of each weight matrix), 16 one-word canary poll in front of the
 * operand polls of tiles off the critical path.  Bits 32 and 64 place the static-walk launches only (the interpreter runs a program as
 * built): 32 deals their tiles without the column-tile placement of bit 4 (with four row tiles, row tile r on XCDs r and r + 4), 64
 * permutes the block index as well, so that the prior half of row tile r sits on XCD r and the posterior half on XCD r + 4; where
 * the deal is not the one the permutation was made for (it needs four row tiles on 256 CUs) a launch is placed as bit 32 says.
 * Bit 128 turns the static walks' look-ahead arming off: by default a static-walk launch of more than four steps stores the
 * sentinels of its polled slabs itself, four steps ahead, from workgroups that wait anyway, and the host fills only the first
 * four steps; with the bit set the host fills every polled slab in front of the launch, as it does for every other launch. */
int blvm_pchain_tune(int bits);
/* The VRNN forward / backward programs at B <= 64 (16-row tiles, fp32, H = Z = 256, R = 512) run on static-walk kernels whose walk is
 * fixed at compile time (mode 1, the default; bit-identical results); mode 0 sends them to the program interpreter, a negative
 * mode only queries.  Returns the mode in effect before the call; mode -2 returns instead how many VRNN programs the process has
 * launched on the static kernels so far, mode -3 how many of those armed their polled slabs themselves (blvm_pchain_tune bit 128). */
int blvm_pchain_static(int mode);
/* Diagnostics: which implementation the single-layer sequence entry points (K4 / K2) took so far in this process.  Copies twelve
 * counters, out[op * 3 + path]: op 0 blvm_lstm_seq_fwd, 1 blvm_lstm_seq_bwd, 2 blvm_gru_seq_fwd, 3 blvm_gru_seq_bwd; path 0 the
 * register-resident persistent kernel, 1 a program of the persistent-chain interpreter, 2 one launch per step.  One count per call
 * (not per launch), taken on the host where the call branches; never touches the device. */
int blvm_rnn_path_counts(unsigned long long out[12]);
/* The same for the RSSM sequence entry points (K5).  Copies six counters: out[0] blvm_rssm_seq_fwd calls that ran as one program of
 * the persistent-chain engine, out[1] those that ran one launch per link and step, out[2] / out[3] the same for blvm_rssm_seq_bwd
 * (one count per call); out[4] / out[5] the linear-link launches of the launch-per-link loops (the backward's initial-state links
 * included) that ran on 16x16 / on 32x32 tiles (one count per launch).  Host-side; never touches the device. */
int blvm_rssm_path_counts(unsigned long long out[6]);
/* The same for the VRNN sequence entry points (K1; blvm_vrnn_seq_fwd / _fwd_dec / _bwd / _bwd_dec).  Copies seven counters: out[0]
 * forward calls that ran as one persistent program (static walk, interpreter or row groups; blvm_pchain_static(-2) tells the static
 * walks apart), out[1] those that ran one launch per link and step, out[2] / out[3] the same for the backward, out[4] the calls of
 * out[0] and out[2] whose program ran on row groups (one count per call); out[5] / out[6] the linear-link launches of the
 * launch-per-link loops that ran on 16x16 / on 32x32 tiles (one count per launch).  Host-side; never touches the device. */
int blvm_vrnn_path_counts(unsigned long long out[7]);
/* The same for the SRNN latent chain (K3; blvm_srnn_latent_fwd / _bwd), laid out as blvm_rssm_path_counts: out[0] / out[1] forward
 * calls on the persistent program / on launch-per-link, out[2] / out[3] the backward, out[4] / out[5] the linear-link launches of
 * the launch-per-link loops (the backward's initial-latent links included) on 16x16 / on 32x32 tiles. */
int blvm_srnn_path_counts(unsigned long long out[6]);
/* Diagnostics / unit test of the persistent-chain engine on its own: L dependent links x_{s+1} = relu(x_s W^T + b), [B,N] x [N,N],
 * as ONE launch.  W16: W [N,N] in the T16 operand layout (blvm_pchain_rows_to_t16 of W: a weight's rows are the "batch");
 * x16: L+1 T16 slabs of ceil(B/16)*16 x N floats, slab 0 = x_0 in T16 (blvm_pchain_rows_to_t16); xs: L row-major [B,N] outputs.
 * nwg: workgroups (0: one per tile, at most one per CU). */
int blvm_pchain_chain_probe(const float* W16, const float* bias, float* x16, float* xs, int B, int N, int L, int nwg, void* stream);
/* The same chain walked by the static-walk kernel (vrnn_static.hip: kinds, flags and K fixed at compile time, pointers and strides
 * from kernel arguments).  N = 256 or 512. */
/* (the weights of a workgroup's tile stay in registers for the launch; _fetch: re-read every link, the form it is priced against) */
int blvm_pchain_static_chain_probe(const float* W16, const float* bias, float* x16, float* xs, int B, int N, int L, int nwg, void* stream);
int blvm_pchain_static_chain_probe_fetch(const float* W16, const float* bias, float* x16, float* xs, int B, int N, int L, int nwg, void* stream);
/* The register-resident form under a poll pacing policy (csrc/pchain.h): the first poll of a tile waits early_delay s_sleep units
   on the waves that leave the previous tile at its barrier and epi_delay on the epilogue waves (0 .. 64 each).  Both zero is
   blvm_pchain_static_chain_probe.  Probe only (tools/probe_static_chain.py --paced). */
int blvm_pchain_static_chain_probe_paced(const float* W16, const float* bias, float* x16, float* xs, int B, int N, int L, int nwg,
                                         int early_delay, int epi_delay, void* stream);
/* dst = T16 operand copy [ceil(B/16)*16, K] of the rows of src [B,K] (row stride ld). */
int blvm_pchain_rows_to_t16(const float* src, int ld, int B, int K, float* dst, void* stream);
/* n host integers -> device memory through kernel arguments (asynchronous on `stream`; a pageable hipMemcpy would block the host
 * until the stream has drained).  Carries the batch's lengths `x_sl` (`blvm/data/batchers.py:145-151` hands them over on the host). */
int blvm_upload_i32(const int32_t* host, int n, int32_t* dst, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * K6  fp32 MFMA GEMM with fused epilogue — replaces nn.Linear(+LeakyReLU/ReLU) chains
 *     (`blvm/models/vrnn.py:487-505` encoder/decoder MLPs; autograd of the same for the backward forms).
 *
 *   C[M,N] (=|+=) epi( sum_k A'(m,k) * B'(k,n) )
 *     op_a = 0: A'(m,k) = A[m*lda + k]      op_a = 1: A'(m,k) = A[k*lda + m]
 *     op_b = 0: B'(k,n) = B[n*ldb + k]      op_b = 1: B'(k,n) = B[k*ldb + n]
 *   epilogue (in this order): + bias[n] (if bias) ; activation act (0 none, 1 ReLU, 2 LeakyReLU(slope)) ;
 *     * dact(gate[m*ldg+n]) (if gate: 1 where gate>0 else slope — derivative of the activation whose OUTPUT is gate)
 *   accumulate != 0: C += result (split_k > 1 forces atomic accumulation; caller zeroes C unless accumulating).
 * ------------------------------------------------------------------------------------------------------------- */
int blvm_gemm_f32(int op_a, int op_b, int M, int N, int K, const float* A, int lda, const float* B, int ldb,
                  float* C, int ldc, const float* bias, int act, float slope, const float* gate, int ldg,
                  int accumulate, int split_k, void* stream);

/* Which kernel family a product takes.  Forward / data-gradient forms with a short reduction and many rows run weight-stationary
 * (csrc/gemm_ws.hip: a wave keeps a 16-column slab of B in registers and streams 16-row blocks of A through the matrix pipe, no LDS);
 * every other product runs on the LDS-staged tiles.  The weight-stationary path is taken when ALL of these hold:
 *   fp32 operands (BLVM_DTYPE_F32), op_a == 0, split_k == 1, no column sums riding along, K % 16 == 0 and 0 < K <= 256, N % 16 == 0,
 *   A 16-byte aligned with lda % 4 == 0, M >= the row threshold.
 * Both paths sum every output as one fp32 fma chain in ascending k: the same product gives the same bits on either.
 *
 * The routing predicate itself, pure host arithmetic (1: weight-stationary, 0: staged tiles): a_addr is A as an integer, has_colsum
 * whether a bias gradient rides on the product, operand a BLVM_DTYPE_* value, min_rows the row threshold to apply. */
int blvm_gemm_ws_route(int op_a, int M, int N, int K, size_t a_addr, int lda, int split_k, int has_colsum, int operand, int min_rows);
/* Sets the row threshold of the process (rows < 0: the built-in value) and returns the one it replaces.  For tests and experiments. */
int blvm_gemm_ws_min_rows(int rows);
/* out[0] = products launched on the staged tiles, out[1] = on the weight-stationary path, since the library was loaded (host
 * counters, no device needed; products that the weight-gradient ring takes are counted in neither). */
int blvm_gemm_path_counts(unsigned long long* out);

/* The kernels ("arms") K6 chooses among, one number per kernel family and tile shape:
 *    0       weight-stationary (gemm_ws_kernel)
 *    1 ..  3 register-staged  64 x  64 tile with fp32 / bf16 / fp16 operands (gemm_kernel / gemm_bf16_kernel)
 *    4 ..  6 register-staged 128 x 128 tile, the same three operand types
 *    7 ..  9 register-staged 128 x 192 tile
 *   10 .. 12 register-staged 192 x 128 tile
 *   13       weight-gradient ring, exact fp32 body (wgrad_exact_kernel: an unsplit request)
 *   14       weight-gradient ring, sliced body (wgrad_kernel)
 *   15       grouped weight gradients on the ring (wgrad_group_kernel)
 *   16       grouped weight gradients on the 64 x 64 tile (gemm_group_kernel)
 * i.e. a staged arm is BLVM_GEMM_ARM_STAGED + 3 * tile + BLVM_DTYPE_*.  BLVM_GEMM_ARMS (17) is the number of arms and, as an
 * answer, "nothing is launched". */
#define BLVM_GEMM_ARM_WS 0
#define BLVM_GEMM_ARM_STAGED 1
#define BLVM_GEMM_ARM_WGRAD_EXACT 13
#define BLVM_GEMM_ARM_WGRAD_SLICED 14
#define BLVM_GEMM_ARM_WGRAD_GROUP 15
#define BLVM_GEMM_ARM_GEMM_GROUP 16
#define BLVM_GEMM_ARMS 17
/* The arm blvm_gemm_f32 launches for a request: pure host arithmetic, no device, and the function blvm_gemm_f32 itself dispatches
 * through.  a_addr / b_addr are A and B as integers (only their low four bits matter), has_bias / has_gate whether the pointers are
 * given, has_colsum whether a bias gradient rides on the product (blvm_wgrad_f32 with db), split_k as REQUESTED, operand a
 * BLVM_DTYPE_* value, min_rows the weight-stationary row threshold to apply.  M == 0 or N == 0: BLVM_GEMM_ARMS. */
int blvm_gemm_arm(int op_a, int op_b, int M, int N, int K, size_t a_addr, int lda, size_t b_addr, int ldb, int split_k, int has_bias,
                  int act, int has_gate, int has_colsum, int operand, int min_rows);
/* The same for blvm_wgrad_group_f32 (arguments as there, addresses as integers, has_dw[i] whether job i has a dW): joins[i] = 1 for
 * the jobs that run together in the grouped launch, 0 for those that go through blvm_gemm_f32 one by one (op_a = op_b = 1, no
 * epilogue, accumulating, the split blvm_wgrad_f32 would choose: blvm_gemm_arm says where), -1 for a job without dW (column sums
 * only).  Returns the arm of the grouped launch, 15 or 16, or BLVM_GEMM_ARMS when there is none (fewer than two jobs fit). */
int blvm_wgrad_group_route(int n, const int* N_out, const int* K_in, int rows, const size_t* d_addr, const int* ldd, const size_t* x_addr,
                           const int* ldx, const int* has_dw, int operand, int* joins);
/* Launches per arm since the library was loaded, out[arm], counted beside each kernel launch and keyed by the kernel launched, not
 * by the answer of the two functions above: on a device the two are checked against each other (tests/test_gpu_gemm_arms.py).
 * Host counters; never touches the device.  Launches that are no GEMM (memsets, column sums) are not counted. */
int blvm_gemm_arm_counts(unsigned long long out[17]);

/* dz[i] = dy[i] * (y[i] > 0 ? 1 : slope) over n contiguous floats: derivative of ReLU / LeakyReLU from its OUTPUT y
 * (used where no producing GEMM exists to fuse it into, e.g. behind the DMoL head).  dz may alias dy. */
int blvm_act_bwd_f32(const float* dy, const float* y, float slope, float* dz, size_t n, void* stream);

/* Weight + bias gradient of y = x W^T + b in ONE launch (autograd's `grad_weight = dy^T x`, `grad_bias = dy.sum(0)`):
 *   dW[n*lddw + k] += sum_r D[r*ldd + n] X[r*ldx + k]   ;   db[n] += sum_r D[r*ldd + n]     (both ACCUMULATE; caller zeroes)
 * D [rows, N_out] pre-activation gradients, X [rows, K_in] the layer's input; dW or db may be NULL; split_k < 1: chosen here.
 * The workgroups of the GEMM's first column block sum the D tiles they stage anyway (fp32 operands; in the bf16-operand mode the
 * bias gradient stays an fp32 sum in its own launch).  Large aligned problems with a split compute fp32-accurate products from three
 * exact bf16 slices per operand; split_k == 1, requested or chosen here (outputs of >= 768 64 x 64 tiles), keeps the exact fp32
 * chain. */
int blvm_wgrad_f32(int N_out, int K_in, int rows, const float* D, int ldd, const float* X, int ldx, float* dW, int lddw, float* db,
                   int split_k, void* stream);

/* n weight (+ bias) gradients over the SAME rows as ONE launch: job i is blvm_wgrad_f32(N_out[i], K_in[i], rows, D[i], ldd[i], X[i],
 * ldx[i], dW[i], lddw[i], db[i]) — the layers of one MLP chain, the links of one recurrent sequence (reference: autograd's per-layer
 * `grad_weight = dy^T x`, torch/nn/functional.linear backward, called once per nn.Linear of blvm/models/vrnn.py:60-75).  Small
 * outputs (256 x 256) cannot fill the chip alone without a split so fine that the atomics dominate; together they share one coarse
 * split.  dW[i] / db[i] may be NULL.  Falls back to one launch per job for 16-bit operands, rows < 1024 or more than 20 jobs. */
int blvm_wgrad_group_f32(int n, const int* N_out, const int* K_in, int rows, const float* const* D, const int* ldd, const float* const* X,
                         const int* ldx, float* const* dW, const int* lddw, float* const* db, void* stream);

/* out[n] (=|+=) sum_m X[m*ldx + n]   (bias gradients). */
int blvm_colsum_f32(int M, int N, const float* X, int ldx, float* out, int accumulate, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * K7  fused DMoL head: Linear(30->30) + split/clamp + discretized-logistic-mixture log-likelihood + mask + per-
 *     utterance sum.  Replaces `blvm/modules/distributions.py:381-387` + `blvm/utils/log_likelihoods.py:170-231`
 *     + the masked sum at `blvm/models/vrnn.py:266-269`.
 *
 *   dec      [rows, S*F] contiguous, F = 3*num_mix features per audio frame (frame f = row*S + j at dec + f*F)
 *   layout   0: rows are batch-major (row = b*Tp + t)   1: rows are time-major (row = t*B + b)
 *   y        [B, T] targets in [-1,1];  x_sl [B] int32 on device;  frame (b, tau=t*S+j) counts iff tau < x_sl[b]
 *   W [F,F], bias [F]: the likelihood's Linear (both NULL: `dec` already holds the F parameters, e.g. WaveNet's
 *   Linear(C->F) computed by K6);  log_eps: clamp floor of the log-scales (-7)
 *   log_prob [B] double, ACCUMULATED (caller zeroes);  ll_twise optional [B,T] fp32 (masked ll, may be NULL):
 *   only the frames t < x_sl[b] are written (caller zeroes: the masked frames keep what they held)
 * ------------------------------------------------------------------------------------------------------------- */
int blvm_dmol_fwd(const float* dec, int layout, const float* W, const float* bias, const float* y,
                  const int32_t* x_sl, int B, int T, int Tp, int S, int num_mix, int num_bins, float log_eps,
                  double* log_prob, float* ll_twise, void* stream);

/*   g_b [B] fp32 = dLoss/dlog_prob[b].  Writes d_dec (same shape as dec; zero on masked frames) and d_par
 *   [rows*S, F] = gradient wrt the Linear's OUTPUT (for dW = d_par^T dec, db = colsum(d_par)). */
int blvm_dmol_bwd(const float* dec, int layout, const float* W, const float* bias, const float* y,
                  const int32_t* x_sl, const float* g_b, int B, int T, int Tp, int S, int num_mix, int num_bins,
                  float log_eps, float* d_dec, float* d_par, void* stream);

/*   The same backward with its two consumers folded in (DMoL, rows path: S % 64 == 0, 16-byte aligned buffers, W given; otherwise
 *   BLVM_NOT_APPLICABLE and nothing is launched).  `dz` = d_dec times the derivative of the activation that produced `dec`
 *   (act_slope >= 0: dec > 0 ? g : g * act_slope, blvm_act_bwd_f32's rule; act_slope < 0: no activation, dz = d_dec).  dW [F,F] =
 *   d_par^T dec and db [F] = column sums of d_par are WRITTEN (either may be NULL; both NULL: no accumulation) — d_par itself is
 *   never stored.  No float atomics: dW and db are identical from run to run.  `workspace`: blvm_dmol_bwd_fused_workspace_floats
 *   floats (0: the shape does not take this path), needed when dW or db is given; its first 256 words are tickets that must be zero
 *   before the first launch and are zero again after every launch; launches that share a workspace must be stream-ordered. */
size_t blvm_dmol_bwd_fused_workspace_floats(int B, int Tp, int S);
int blvm_dmol_bwd_fused(const float* dec, int layout, const float* W, const float* bias, const float* y,
                        const int32_t* x_sl, const float* g_b, int B, int T, int Tp, int S, int num_mix, int num_bins,
                        float log_eps, float act_slope, float* dz, float* dW, float* db, float* workspace, void* stream);

/* K7b / K7c  Gaussian output heads, same calling convention, frame layout, masks and float64 per-utterance sums as K7:
 *   gmm: `DiagonalGaussianMixtureDense.forward` + `.log_prob` (`blvm/modules/distributions.py:153-206`,
 *        `gaussian_mixture_ll` `blvm/utils/log_likelihoods.py:42-60`): dec [rows, S*3*num_mix] -> Linear(3 num_mix -> 3 num_mix) (W
 *        NULL: dec ARE the parameters) -> logits | means | pre-softplus sds, sd = softplus_beta(raw) + sd_eps.  1 <= num_mix <= 16
 *        (anything else: an error before any launch); ten components run the kernels of the audio models, any other count a
 *        general arm at frame width 3 num_mix.
 *   gauss_head: `DiagonalGaussianDense.forward` + `.log_prob` (`distributions.py:105-150`, `gaussian_ll`
 *        `log_likelihoods.py:17-39`): dec [rows, S*2] -> Linear(2->2) (W NULL: none) -> mean | pre-softplus sd.
 *   bwd: d_dec (gradient wrt dec) and d_par (gradient wrt the Linear's output; dW = d_par^T dec, db = colsum(d_par)). */
int blvm_gmm_fwd(const float* dec, int layout, const float* W, const float* bias, const float* y, const int32_t* x_sl,
                 int B, int T, int Tp, int S, int num_mix, float sd_beta, float sd_eps, double* log_prob, float* ll_twise,
                 void* stream);
int blvm_gmm_bwd(const float* dec, int layout, const float* W, const float* bias, const float* y, const int32_t* x_sl,
                 const float* g_b, int B, int T, int Tp, int S, int num_mix, float sd_beta, float sd_eps, float* d_dec,
                 float* d_par, void* stream);
int blvm_gauss_head_fwd(const float* dec, int layout, const float* W, const float* bias, const float* y,
                        const int32_t* x_sl, int B, int T, int Tp, int S, float sd_beta, float sd_eps, double* log_prob,
                        float* ll_twise, void* stream);
int blvm_gauss_head_bwd(const float* dec, int layout, const float* W, const float* bias, const float* y,
                        const int32_t* x_sl, const float* g_b, int B, int T, int Tp, int S, float sd_beta, float sd_eps,
                        float* d_dec, float* d_par, void* stream);

/* Samplers / modes of the mixture heads (`DiscretizedLogisticMixtureDense.sample/.mode`, `DiagonalGaussianMixtureDense.sample/.mode`,
 * `blvm/modules/distributions.py:173-186,359-368`; `blvm/utils/variational.py:156-195,283-349`).  par [n, 3*num_mix] = head outputs
 * (logits | locations | raw scales); u [n,num_mix] uniforms for the Gumbel-max component pick (NULL: arg-max logit = mode);
 * v [n] the picked component's noise (kind 0 DMoL: uniform -> logistic, clamped to [-1,1]; kind 1 GMM: standard normal;
 * NULL: the location).  out [n].  The caller draws u, v (RNG stays with the host framework, as for eps). */
int blvm_mix_sample(const float* par, const float* u, const float* v, long long n, int num_mix, int kind, float log_eps,
                    float sd_beta, float sd_eps, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * K7d  categorical (softmax) head fused with its Linear(C -> V): `CategoricalDense.forward` + `.log_prob(..., reduce_dim=None)`
 *      (`blvm/modules/distributions.py:207-235`, `categorical_ll` `blvm/utils/log_likelihoods.py:63-80`: logits - logsumexp, gather
 *      at y) + the mask and per-utterance sum of `blvm/models/wavenet/wavenet.py:128-146`.  The [frames, V] logits are never
 *      stored: tiles of them are recomputed on the exact-fp32 matrix pipe wherever they are needed.
 *
 *   dec   [rows, S*C] contiguous, rows TIME-MAJOR (row = t*B + b), rows = Tp*B; frame (b, tau = t*S + j) at dec + (row*S + j)*C
 *   W [V, C], bias [V]: the head's Linear;  y [B, T] int32 classes;  x_sl [B] int32 on device
 *   frame (b, tau) counts iff tau < min(x_sl[b], T).  A frame that does not count changes nothing, whatever its target (any
 *   integer) and its activations (NaN included) hold.  A counted frame whose target lies outside [0, V) has ll = -inf: the target is
 *   compared with the class index and never used as an address.
 *   Shapes: C % 16 == 0, 16 <= C <= 512, 2 <= V <= 65536 (else BLVM_ENOSUP); dec, W, d_dec, dW 16-byte aligned.  Operands are fp32
 *   whatever blvm_set_operand_dtype says, as for K7.
 *   fwd: lse [rows*S] fp32 (log-sum-exp of the frame's logits, 0 where the frame does not count), ll [B, T] fp32 (l_y - lse, 0 where
 *   the frame does not count; every element is written), log_prob [B] double ACCUMULATED (caller zeroes; may be NULL): the float64
 *   sum of ll[b, :] in a fixed order. */
int blvm_cat_fwd(const float* dec, const float* W, const float* bias, const int32_t* y, const int32_t* x_sl, int B, int T, int Tp, int S,
                 int C, int V, float* lse, float* ll, double* log_prob, void* stream);

/*   Backward of log_prob (autograd through `logits.logsumexp` / `.gather`, log_likelihoods.py:75-79, and nn.Linear): with
 *   d = g_b[b] * mask * (onehot(y) - exp(l - lse)) per frame, recomputed tile by tile from dec, W and the forward's `lse`,
 *   d_dec [rows, S*C] = d W (zero on frames that do not count), dW [V, C] = d^T dec, db [V] = column sums of d: all WRITTEN; any of
 *   the three may be NULL.  d itself never reaches global memory.  No float atomics: repeated calls give identical bits.
 *   `workspace`: blvm_cat_bwd_workspace_floats(rows*S, C, V) floats (may be uninitialised; NULL when that is 0, or when dW and db are
 *   NULL): partial dW / db of the row splits that fill the chip when V is small (V >= 16384: none) — under
 *   2^15 * (C + 1) floats whatever the number of frames. */
size_t blvm_cat_bwd_workspace_floats(long long frames, int C, int V);
int blvm_cat_bwd(const float* dec, const float* W, const float* bias, const int32_t* y, const int32_t* x_sl, const float* lse,
                 const float* g_b, int B, int T, int Tp, int S, int C, int V, float* d_dec, float* dW, float* db, float* workspace,
                 void* stream);

/*   Draws / modes of the head on materialised logits [n, V] (`CategoricalDense.sample` / `.mode`, distributions.py:223-229:
 *   `torch.distributions.Categorical(logits).sample()`, `torch.argmax`).  u NULL: the arg-max, the lowest index on a tie.  Otherwise
 *   u [n] uniforms and the inverse CDF: with m = max l, e_k = exp(l_k - m), S = sum e, out = the smallest k whose running sum
 *   e_0 + .. + e_k reaches u * S (V - 1 if none does).  out [n] int32.  The caller draws u, as for blvm_mix_sample. */
int blvm_cat_sample(const float* logits, const float* u, long long n, int V, int32_t* out, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * K8  fused analytic Gaussian KL + free-nats + mask + per-utterance sums.  Replaces
 *     `blvm/utils/variational.py:67-70,86-122` + `blvm/models/vrnn.py:271-276`.
 *   mu_q, sd_q, mu_p, sd_p [rows=Tp*B, Z] (layout as above); step t of row b counts iff t*stride < x_sl[b]
 *   fn_floor = free_nats / Z (<= 0 disables);  kld, kld_fn [B] double, ACCUMULATED (caller zeroes)
 * ------------------------------------------------------------------------------------------------------------- */
int blvm_kl_fwd(const float* mu_q, const float* sd_q, const float* mu_p, const float* sd_p, int layout,
                const int32_t* x_sl, int B, int Tp, int Z, int stride, float fn_floor, double* kld,
                double* kld_fn, void* stream);

/*   c_raw[b] = dLoss/dkld[b], c_fn[b] = dLoss/dkld_fn[b] (fp32, either may be NULL = 0). */
int blvm_kl_bwd(const float* mu_q, const float* sd_q, const float* mu_p, const float* sd_p, int layout,
                const int32_t* x_sl, const float* c_raw, const float* c_fn, int B, int Tp, int Z, int stride,
                float fn_floor, float* d_mu_q, float* d_sd_q, float* d_mu_p, float* d_sd_p, void* stream);

/* ELBO assembly from the per-utterance float64 sums (`compute_elbo`, `blvm/models/vrnn.py:266-279`), one launch:
 *   elbo[b] = log_prob[b] - kld[b];  *loss = -(sum_b log_prob[b] - beta kld_fn[b]) / n_frames;
 *   sums [4] = (loss, sum elbo, sum log_prob, sum kl) with kl = kld_fn (kl_raw 0) or kld (kl_raw 1); sums in a fixed order over b. */
int blvm_elbo_fwd(const double* log_prob, const double* kld, const double* kld_fn, double beta, double n_frames, int B,
                  int kl_raw, double* elbo, double* loss, double* sums, void* stream);
/*   g_loss: the float64 scalar gradient of loss ON THE DEVICE (NULL = 0), g_elbo [B] that of elbo (NULL = 0).  Writes the gradients
 *   of (log_prob | kld_fn | kld) as g64 [3,B] float64 and, rounded, as g32 [3,B] float32 (what the backward kernels of K7 / K1 read). */
int blvm_elbo_bwd(const double* g_loss, const double* g_elbo, double beta, double n_frames, int B, double* g64, float* g32,
                  void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * K8m  the reductions of the K-sample importance-weighted bound L_K = log (1/K) sum_k p(x, z_k) / q(z_k | x), z_k ~ q (evaluation
 *      only, no backward; an addition beyond the reference, which reports the single-sample ELBO).
 * blvm_gauss_logratio_fwd: the Monte-Carlo log-density ratio at the drawn z.  All six inputs [rows=Tp*B, Z] fp32 in the layouts and
 *   with the mask of blvm_kl_fwd (step t of row b counts iff t*stride < x_sl[b]).  Per element
 *     r = log(sd_p) - log(sd_q) - eps^2 / 2 + ((z - mu_p) / sd_p)^2 / 2
 *   (the q-term from eps: z - mu_q = sd_q eps is how z was drawn, so mu_q is not read; the p-term from the stored z, the value the
 *   decoder saw).  out[b] = the float64 sum of r over the live steps and all Z elements of row b, WRITTEN (not accumulated): every
 *   word of out is written (a row with x_sl[b] = 0 gets 0), the result does not depend on the prior contents of out, masked steps
 *   are not read, and calls are bit-identical (fixed reduction order, no floating-point atomics).  Any Z >= 1 and any alignment:
 *   16-byte loads where Z % 4 == 0 and the bases are aligned, a scalar path otherwise.  BLVM_EINVAL before any launch on a null
 *   pointer, B, Tp, Z or stride < 1, a layout other than 0 or 1.
 * blvm_iw_reduce: log_w [K,B] float64 -> with m = max_k log_w[k,b] and w = exp(log_w - m):
 *     bound[b] = m + log sum_k w - log K,   ess[b] = (sum_k w)^2 / sum_k w^2   (ess may be NULL)
 *   summed over k in ascending order (calls are bit-identical).  A column of all -inf gives bound = -inf, ess = 0; a NaN anywhere in
 *   a column gives NaN in that column only.  K = 1 returns log_w itself, K equal weights return that weight and ess = K, exactly.
 * ------------------------------------------------------------------------------------------------------------- */
int blvm_gauss_logratio_fwd(const float* mu_q, const float* sd_q, const float* mu_p, const float* sd_p, const float* z,
                            const float* eps, int layout, const int32_t* x_sl, int B, int Tp, int Z, int stride, double* out,
                            void* stream);
int blvm_iw_reduce(const double* log_w, int K, int B, double* bound, double* ess, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * K8r  the last launch of every `represent()` level (evaluation only, no backward): the mean of the latents over particles with the
 *      frames past each utterance's length zeroed.  z [T, c*B, Z] fp32 time-major with row k*B + b (particle k of utterance b, as the
 *      iw_bound passes lay their rows), lens [B] in frames of this level, out [T, B, Z].  Per element
 *        acc = first ? 0 : out;   acc += z[t, k*B+b, :] for k = 0 .. c-1, one fp32 add each;
 *        out = last ? (t < lens[b] ? acc * scale : 0) : acc
 *      so K particles split over any passes (first on the first, last and scale = 1/K on the last) are ONE chain of fp32 adds in
 *      particle order: bit-identical for every split and from call to call.  c = 1, first = last = 1, scale = 1 is z itself with the
 *      dead frames +0, whatever z held there.  With first = 1 no word of out depends on its previous contents and every word is
 *      written.  Streaming: 16-byte loads and stores, grid-stride, no LDS, no atomics.  BLVM_EINVAL before any launch on a null
 *      pointer, T, B or Z < 1, c < 1, Z % 4 != 0, z or out not 16-byte aligned.
 * ------------------------------------------------------------------------------------------------------------- */
int blvm_particle_mean(const float* z, const int32_t* lens, int T, int c, int B, int Z, int first, int last, float scale,
                       float* out, void* stream);

/* K8b  Gaussian latent head, elementwise over n = rows*Z: sd = softplus_beta(raw) + sd_eps for prior and posterior
 * (`DiagonalGaussianDenseSTCN.forward`, `blvm/models/stcn/stcn.py:32-76`), posterior combination (mode 0 plain, 1 residual
 * mu_q += mu_p, 2 precision-weighted `variational.py:125-138`) and the reparameterised sample z = mu_q + sd_q*eps
 * (`variational.py:141-152`) — the per-level body of `STCN.infer` (`stcn.py:297-327`).  bwd: upstream gradients wrt the four
 * outputs (each may be NULL) -> gradients wrt mu_p, sd_p_raw, mu_q_raw, sd_q_raw. */
int blvm_gauss_latent_fwd(const float* mu_p, const float* sd_p_raw, const float* mu_q_raw, const float* sd_q_raw,
                          const float* eps, size_t n, float beta_p, float beta_q, float sd_eps, int mode, float* sd_p,
                          float* mu_q, float* sd_q, float* z, void* stream);
int blvm_gauss_latent_bwd(const float* mu_p, const float* sd_p_raw, const float* mu_q_raw, const float* sd_q_raw,
                          const float* eps, const float* g_sd_p, const float* g_mu_q, const float* g_sd_q, const float* g_z,
                          size_t n, float beta_p, float beta_q, float sd_eps, int mode, float* d_mu_p, float* d_sd_p_raw,
                          float* d_mu_q_raw, float* d_sd_q_raw, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * K1  VRNN recurrent cell over a whole sequence (forward and BPTT).  Replaces the scripted per-step loop
 *     `blvm/models/vrnn.py:305-308` over `VRNNCell.forward` (`vrnn.py:109-141`) and its autograd backward.
 *     condition_h_on_x = True (the only form VRNNAudio builds, `vrnn.py:506-516`).
 *
 *   weights: reference layout, Linear [out,in], GRU rows [r|z|n] (`SURVEY.md` §8b).
 *   X = x_dim (encoder feature size), H = h_dim (MLP width), Z = z_dim, R = r_dim (GRU state).
 *   All of X, H, Z, R must be multiples of 16; B is arbitrary (row-guarded tiles).
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct BlvmVrnnWeights {
  const float *prior_w[3], *prior_b[3]; /* [H,R], [H,H], [H,H] */
  const float *prior_hw, *prior_hb;     /* [2Z,H] */
  const float *post_w[3], *post_b[3];   /* [H,R+X] (input order cat[h,x]), [H,H], [H,H] */
  const float *post_hw, *post_hb;       /* [2Z,H] */
  const float *phi_w[4], *phi_b[4];     /* [H,Z], [H,H] x3 */
  const float *gru_wih, *gru_whh;       /* [3R, X+H] (input order cat[x,phi]), [3R,R] */
  const float *gru_bih, *gru_bhh;       /* [3R] */
} BlvmVrnnWeights;

typedef struct BlvmVrnnGrads { /* same shapes as the weights; ACCUMULATED into (caller zeroes) */
  float *prior_w[3], *prior_b[3], *prior_hw, *prior_hb;
  float *post_w[3], *post_b[3], *post_hw, *post_hb;
  float *phi_w[4], *phi_b[4];
  float *gru_wih, *gru_whh, *gru_bih, *gru_bhh;
} BlvmVrnnGrads;

/* K1c  Ancestral sampling from VRNNAudio: every step of every utterance in ONE launch.  Replaces the loop of `VRNN.generate`
 *   (`blvm/models/vrnn.py:371-434`): enc = encoder(x_t) -> `VRNNCell.generate` (`vrnn.py:143-164`: prior -> z = mu + sd eps ->
 *   phi_z -> GRU) -> decoder(cat[phi_z, h_new]) -> DMoL head per sample -> draw -> x_{t+1}.  All weights in their PyTorch layouts;
 *   the encoder / decoder are 3 x (Linear + LeakyReLU(slope)) as in `vrnn.py:487-505`, x_dim = H.
 *   x0 [B,S] first frame stack; h0 [B,R] or NULL (zeros); eps [T,B,Z] standard normal; u [T,B,S,num_mix], v [T,B,S] uniforms of the
 *   DMoL sampler as in blvm_mix_sample (both NULL: the mode); x_out [B,T,S]; h_out [B,R] or NULL.
 *   scratch: blvm_vrnn_decode_scratch_floats(...) floats (operand-layout copies of the weights). */
typedef struct BlvmVrnnDecodeWeights {
  const float *enc_w[3], *enc_b[3]; /* [H,S], [H,H], [H,H] */
  const BlvmVrnnWeights* cell;      /* prior_*, phi_*, gru_* are read (the posterior is not evaluated when z comes from the prior) */
  const float *dec_w[3], *dec_b[3]; /* [H,H+R] (input order cat[phi_z, h]), [H,H], [S*3*num_mix,H] */
  const float *lik_w, *lik_b;       /* [3*num_mix, 3*num_mix], [3*num_mix]: the head's Linear, applied per sample */
} BlvmVrnnDecodeWeights;
size_t blvm_vrnn_decode_scratch_floats(int S, int H, int Z, int R);
int blvm_vrnn_decode(const BlvmVrnnDecodeWeights* w, const float* x0, const float* h0, const float* eps, const float* u,
                     const float* v, int T, int B, int S, int H, int Z, int R, int num_mix, float sd_eps, float slope,
                     float log_eps, float* x_out, float* h_out, float* scratch, void* stream);

/* K1c on the whole chip: the same sampling loop (same arguments and draws, B <= 128) as ONE persistent launch whose every layer is a
 * link dealt over all CUs (csrc/pchain.hip) instead of 16 utterances per CU: 17 links per step.  scratch:
 * blvm_vrnn_generate_scratch_floats(T, B, ...) floats (weight copies + one slab per step of every activation).
 * The frame stack may have any size S >= 1 (H, Z, R multiples of 16, num_mix = 10; blvm_vrnn_decode keeps S % 16 == 0).  When S is no
 * multiple of 16 the launch works on padded copies inside the scratch, and the *_scratch_floats functions return the padded sizes: the
 * frame-stack operand is Sp = 16 ceil(S / 16) wide (zero weight columns), the last decoder layer's output rows are Np =
 * 16 ceil(S 3 num_mix / 16) floats long (zero weight rows, a zero-padded copy of its bias).  x0, x_out, u and v keep width S; nothing
 * of the caller's is read past its end.  The same rule holds for blvm_srnn_generate and blvm_lstm_generate_any_stack.  The scratch grows with T
 * and the step program does not depend on T: a long roll-out may be run as consecutive calls, each from the previous call's last frame
 * stack and state, with bit-identical results (blvm.ops does so above `MAX_SCRATCH_FLOATS`). */
size_t blvm_vrnn_generate_scratch_floats(int T, int B, int S, int H, int Z, int R);
int blvm_vrnn_generate(const BlvmVrnnDecodeWeights* w, const float* x0, const float* h0, const float* eps, const float* u,
                       const float* v, int T, int B, int S, int H, int Z, int R, int num_mix, float sd_eps, float slope,
                       float log_eps, float* x_out, float* h_out, float* scratch, void* stream);

/* The head of a roll-out's draw: what the last link of every step does with the head Linear's outputs of one sample.  The header's
 * structs hold pointers only (the bindings are generated from them), so a head is five scalars, always in this order:
 *   head_kind, num_mix, log_eps, head_sd_beta, head_sd_eps
 *   kind 0  DMoL      outputs logits | locations | raw log-scales (num_mix each): the draw of blvm_mix_sample kind 0 (log_eps);
 *                     the two head_sd_* are not read
 *   kind 1  GMM       outputs logits | means | raw scales (num_mix each): the draw of blvm_mix_sample kind 1, sd = softplus_beta(raw)
 *                     + head_sd_eps with beta = head_sd_beta (0: raw is the sd); u as for kind 0, v [T,B,S] STANDARD NORMALS; no clamp
 *   kind 2  Gaussian  outputs (mean, raw scale): x = mean + sd v with the same sd, no component pick: u must be NULL, v [T,B,S]
 *                     standard normals or NULL (x = the mean); num_mix and log_eps are not read
 * Kinds 0 and 1 take u and v together (both NULL: the arg-max-logit component's location).  With F = 3 num_mix (kinds 0, 1) or F = 2
 * (kind 2): the last decoder layer is [S*F, H], its bias [S*F], lik_w [F,F], lik_b [F], and where S is no multiple of 16 the padded
 * row of the last layer is Np = 16 ceil(S F / 16) floats.  Refused with BLVM_EINVAL before any launch or write: a kind other than
 * 0, 1, 2; num_mix != 10 for kinds 0 and 1; head_sd_beta < 0; u given for kind 2.
 *
 * K1c with a head: blvm_vrnn_decode and blvm_vrnn_generate are the kind-0 cases (0, num_mix, log_eps, 0, 0) of these calls, which
 * take the same arguments in the same layouts with the head in place of `num_mix, log_eps` (sd_eps and slope stay the cell's and the
 * MLPs').  The per-CU form blvm_vrnn_decode_head draws kinds 0 and 1 (kind 2 is refused, as every refusal before any launch or
 * write); its scratch does not depend on the head: blvm_vrnn_decode_scratch_floats.  The whole-chip form draws all three; its scratch
 * depends on F: blvm_vrnn_generate_scratch_floats_head (0 for a kind it does not draw).  Caller-owned buffers as for the calls above:
 * every word of scratch that is read is written first by the same call, results do not depend on the prior contents of scratch or of
 * the outputs, and nothing outside x_out, h_out and scratch is written. */
size_t blvm_vrnn_generate_scratch_floats_head(int T, int B, int S, int H, int Z, int R, int head_kind);
/* 1 when the per-CU form takes these widths (multiples of 16 within its op-program, state-tile and LDS limits), else 0: what a caller
 * asks before it draws noise for a batch above blvm_pchain_max_batch().  Host arithmetic, no GPU call. */
int blvm_vrnn_decode_applies(int S, int H, int Z, int R);
int blvm_vrnn_generate_head(const BlvmVrnnDecodeWeights* w, const float* x0, const float* h0, const float* eps, const float* u,
                            const float* v, int T, int B, int S, int H, int Z, int R, int head_kind, int num_mix, float log_eps,
                            float head_sd_beta, float head_sd_eps, float sd_eps, float slope, float* x_out, float* h_out,
                            float* scratch, void* stream);
int blvm_vrnn_decode_head(const BlvmVrnnDecodeWeights* w, const float* x0, const float* h0, const float* eps, const float* u,
                          const float* v, int T, int B, int S, int H, int Z, int R, int head_kind, int num_mix, float log_eps,
                          float head_sd_beta, float head_sd_eps, float sd_eps, float slope, float* x_out, float* h_out,
                          float* scratch, void* stream);

/* number of floats of `reserve` (activations kept for BPTT) / `workspace` (backward scratch). */
size_t blvm_vrnn_reserve_floats(int Tp, int B, int X, int H, int Z, int R);
size_t blvm_vrnn_bwd_workspace_floats(int Tp, int B, int X, int H, int Z, int R);

/*   enc [Tp,B,X]; h0 [B,R] (NULL = zeros); eps [Tp,B,Z] standard-normal noise (reference draws it per step,
 *   `blvm/utils/variational.py:141-152`); sd_eps = epsilon of the Gaussian heads (1e-6), initial_sd = 1.
 *   decin [Tp+1,B,H+R]: row t = [phi_t | h_{t-1}] — the decoder input `cat([phi_z, h])` of `vrnn.py:321-324`;
 *     row Tp carries the final state in its h-part; its phi-part (there is no step Tp) is written as zeros.
 *   mu_q (residual already added), sd_q, mu_p, sd_p, z: [Tp,B,Z]. */
int blvm_vrnn_seq_fwd(const BlvmVrnnWeights* w, const float* enc, const float* h0, const float* eps, int Tp, int B,
                      int X, int H, int Z, int R, int residual_posterior, float sd_eps, float* decin,
                      float* mu_q, float* sd_q, float* mu_p, float* sd_p, float* z, float* reserve, void* stream);

/* The same forward with the decoder MLP of `vrnn.py:321-324` (3 x (Linear + LeakyReLU(slope)) on decin rows 0 .. Tp-1) handed down:
 * where the launch has workgroups to spare (fp32 operands, B <= 64 on 16-row tiles, Z == H, DH == H, SF a multiple of 16, and the
 * deal of csrc/vrnn_static.h leaves a decoder range) the three layers run inside the persistent forward launch as a follower of the
 * chain and *folded = 3: dec_y[0] [Tp*B,DH], dec_y[1] [Tp*B,DH] and dec_y[2] [Tp*B,SF] then hold the three activations.  Otherwise
 * *folded = 0, they are not written and the caller runs the decoder itself (K6).  Everything else is computed exactly as by
 * blvm_vrnn_seq_fwd.  dec_w, dec_b, dec_y: host arrays of three device pointers each.
 *   dec_w[0] [DH,H+R] (input order cat[phi_z, h]), dec_w[1] [DH,DH], dec_w[2] [SF,DH]; SF = S * (the head's features per sample).
 *   reserve: blvm_vrnn_fwd_reserve_floats(..., DH, SF) floats, asked for under the same blvm_vrnn_dec_fold mode as the call (more than
 *   blvm_vrnn_reserve_floats only where the call folds); blvm_vrnn_seq_bwd reads it as it reads blvm_vrnn_seq_fwd's.
 * *folded = 2: the first two layers only (dec_y[2] is not written; the caller runs the last layer on dec_y[1]).
 * blvm_vrnn_dec_fold(mode): 0 never folds, 1 (default; env BLVM_VRNN_DEC_FOLD) folds where it applies, 2 folds the first two layers
 * only, negative only queries;
 * returns the mode in effect before the call, mode -2 instead the number of forward calls that folded so far. */
size_t blvm_vrnn_fwd_reserve_floats(int Tp, int B, int X, int H, int Z, int R, int DH, int SF);
int blvm_vrnn_seq_fwd_dec(const BlvmVrnnWeights* w, const float* enc, const float* h0, const float* eps, int Tp, int B,
                          int X, int H, int Z, int R, int residual_posterior, float sd_eps, float* decin,
                          float* mu_q, float* sd_q, float* mu_p, float* sd_p, float* z, float* reserve,
                          const float* const* dec_w, const float* const* dec_b, float* const* dec_y, int DH, int SF, float slope,
                          int* folded, void* stream);
int blvm_vrnn_dec_fold(int mode);

/*   d_decin [Tp+1,B,H+R]: gradient wrt decin (row Tp ignored).  KL term folded in: loss += sum_b (c_raw[b] *
 *   kld[b] + c_fn[b] * kld_fn[b]) with the mask t*stride < x_sl[b] and floor fn_floor (see blvm_kl_fwd);
 *   c_raw / c_fn may be NULL (= 0).
 *   Outputs: d_enc [Tp,B,X], d_h0 [B,R] (may be NULL), grads (accumulated). */
int blvm_vrnn_seq_bwd(const BlvmVrnnWeights* w, const float* enc, const float* eps, const float* decin,
                      const float* mu_q, const float* sd_q, const float* mu_p, const float* sd_p, const float* z,
                      const float* reserve, const float* d_decin, const int32_t* x_sl, const float* c_raw,
                      const float* c_fn, int stride, float fn_floor, int Tp, int B, int X, int H, int Z, int R,
                      int residual_posterior, float sd_eps, float* d_enc, float* d_h0, const BlvmVrnnGrads* grads,
                      float* workspace, void* stream);

/* The same backward with the decoder MLP's data gradients handed down (the mirror image of blvm_vrnn_seq_fwd_dec): where the backward
 * launch has a spare range (the conditions of the forward fold and in addition H == 256, R == 512, the split3 program on its own-range
 * deal, Tp >= 4) the three products dY2 = gate(dZ3 Wd3), dY1 = gate(dY2 Wd2), d_decin = dY1 Wd1 run inside the persistent launch,
 * a fixed number of steps ahead of the chain, and *folded = 1.  Otherwise *folded = 0 and NOTHING has been done: the caller runs the
 * decoder's data gradients itself (K6) and calls blvm_vrnn_seq_bwd.  There is no d_decin argument: a gradient that reaches decin from
 * anywhere but the decoder is the caller's reason to take that path.
 *   dz3 [Tp*B,SF]: gradient of the decoder's last PRE-activation (what blvm_dmol_bwd_fused returns with act_slope >= 0);
 *   dec_y1, dec_y2 [Tp*B,DH]: the decoder's hidden activations; dec_w: host array of the three weight pointers (as for the forward);
 *   dy2, dy1 [Tp*B,DH] (out): gradients of the hidden pre-activations, every row written; the decoder's weight gradients are the
 *   caller's (dW3 = dz3^T y2, dW2 = dy2^T y1, dW1 = dy1^T decin).
 *   workspace: blvm_vrnn_bwd_dec_workspace_floats(..., DH, SF) floats, asked for under the same blvm_vrnn_dec_bwd_fold mode.
 * blvm_vrnn_dec_bwd_fold(mode): 0 never folds, 1 (default; env BLVM_VRNN_DEC_BWD_FOLD) folds where it applies, negative only queries;
 * returns the mode in effect before the call, mode -2 instead the number of backward calls that folded so far. */
size_t blvm_vrnn_bwd_dec_workspace_floats(int Tp, int B, int X, int H, int Z, int R, int DH, int SF);
int blvm_vrnn_seq_bwd_dec(const BlvmVrnnWeights* w, const float* enc, const float* eps, const float* decin,
                          const float* mu_q, const float* sd_q, const float* mu_p, const float* sd_p, const float* z,
                          const float* reserve, const int32_t* x_sl, const float* c_raw, const float* c_fn, int stride,
                          float fn_floor, int Tp, int B, int X, int H, int Z, int R, int residual_posterior, float sd_eps,
                          float* d_enc, float* d_h0, const BlvmVrnnGrads* grads, float* workspace, const float* dz3,
                          const float* dec_y1, const float* dec_y2, const float* const* dec_w, float* dy2, float* dy1, int DH,
                          int SF, float slope, int* folded, void* stream);
int blvm_vrnn_dec_bwd_fold(int mode);

/* d_enc inside the backward launch: where blvm_vrnn_seq_bwd / blvm_vrnn_seq_bwd_dec are asked for d_enc and the walk is the static
 * split3 one (fp32 operands, B <= 64 on 16-row tiles, X == H == Z == 256, R == 512, the own-range deal with one tile of [B, X] for
 * every workgroup of the posterior half, Tp >= 5), d_enc = DQ0 Wq0[:, R:] + DGI W_ih[:, :X] is computed on the walk's posterior half,
 * one walk step behind the chain, every word written once; otherwise as two K6 products behind the launch, the second accumulating
 * into the first.  blvm_vrnn_bwd_workspace_floats and blvm_vrnn_bwd_dec_workspace_floats grow where a call would fold: ask for the
 * workspace under the same mode as the call.
 * blvm_vrnn_enc_bwd_fold(mode): 0 never folds, 1 (default; env BLVM_VRNN_ENC_BWD_FOLD) folds where it applies, negative only queries;
 * returns the mode in effect before the call, mode -2 instead the number of backward calls that folded so far. */
int blvm_vrnn_enc_bwd_fold(int mode);

/* ---------------------------------------------------------------------------------------------------------------
 * K4  single-layer LSTM over a sequence (forward + BPTT).  Replaces `nn.LSTM` on a packed sequence,
 *     `blvm/models/lstm.py:46-55,96-98` (pack_padded_sequence / pad_packed_sequence semantics through `lens`:
 *     a row past its length keeps its state and emits zeros).  Gate rows [i|f|g|o].
 *   in [T,B,I]; h0,c0 [B,H] or NULL (zeros); lens [B] int32 valid steps per row, or NULL (all T)
 *   out [T,B,H]; hn,cn [B,H] state after each row's last valid step (may be NULL)
 * ------------------------------------------------------------------------------------------------------------- */
size_t blvm_lstm_reserve_floats(int T, int B, int H);
size_t blvm_lstm_bwd_workspace_floats(int T, int B, int H);
int blvm_lstm_seq_fwd(const float* Wih, const float* Whh, const float* bih, const float* bhh, const float* in,
                      const float* h0, const float* c0, const int32_t* lens, int T, int B, int I, int H, float* out,
                      float* hn, float* cn, float* reserve, void* stream);
/*   d_out [T,B,H]; outputs d_in [T,B,I], d_h0, d_c0 [B,H] (each may be NULL); weight grads ACCUMULATED (may be NULL). */
int blvm_lstm_seq_bwd(const float* Wih, const float* Whh, const float* in, const float* reserve, const float* d_out,
                      int T, int B, int I, int H, float* d_in, float* d_h0, float* d_c0, float* dWih, float* dWhh,
                      float* dbih, float* dbhh, float* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * K4b  one BIDIRECTIONAL LSTM layer over a sequence (forward + BPTT), both directions in ONE persistent launch.
 *     Replaces the bidirectional `nn.LSTM` layer on a packed sequence inside `LSTMBlock.forward`,
 *     `blvm/modules/lstm_block.py:60-82`.  The reverse direction is the per-row time reversal of K2: row b consumes
 *     time index lens[b]-1-j at recurrence step j < lens[b] (index j in its right padding, where it is not live) and
 *     writes its output at that time index.  Gate rows [i|f|g|o]; the two directions' parameters stay separate, in
 *     their PyTorch layouts (`weight_ih_l0`, `weight_ih_l0_reverse`, ...: `_f` / `_r` below).  Initial states are
 *     zero; no final states are returned and no initial-state gradient is computed.
 *   in [T,B,I]; lens [B] int32 valid steps per row (required; any order, 0 allowed)
 *   out [T,B,2H]: forward direction in columns [0,H), reverse in [H,2H), zeros past a row's length in both halves
 *   The one-launch form takes T >= 4, B <= 128, H in {128, 256, 384} on a device of at least 32 CUs that holds all
 *   2 (H/16) ceil(B/16) workgroups at once.  Any other shape returns BLVM_NOT_APPLICABLE before anything is
 *   written or launched: run two K4 calls instead.  blvm_lstm_bidir_applies answers 1 / 0 for a shape on the
 *   current device without touching it, so a caller need not allocate for a call that would be refused.  The
 *   two size functions are host arithmetic for any shape (for B > 128 they omit, like K4's, the operand slabs).
 *   blvm_lstm_bidir_path_counts: out[0] / out[1] = forward / backward calls so far that ran the one-launch
 *   kernels; these calls never move the counters of blvm_rnn_path_counts.
 * ------------------------------------------------------------------------------------------------------------- */
size_t blvm_lstm_bidir_reserve_floats(int T, int B, int H);
size_t blvm_lstm_bidir_bwd_workspace_floats(int T, int B, int H);
int blvm_lstm_bidir_fwd(const float* Wih_f, const float* Whh_f, const float* bih_f, const float* bhh_f,
                        const float* Wih_r, const float* Whh_r, const float* bih_r, const float* bhh_r, const float* in,
                        const int32_t* lens, int T, int B, int I, int H, float* out, float* reserve, void* stream);
/*   d_out [T,B,2H] (its values past a row's length are ignored); d_in [T,B,I] = the sum of both directions'
 *   contributions (may be NULL); the eight weight / bias grads ACCUMULATED (each may be NULL). */
int blvm_lstm_bidir_bwd(const float* Wih_f, const float* Whh_f, const float* Wih_r, const float* Whh_r, const float* in,
                        const int32_t* lens, const float* reserve, const float* d_out, int T, int B, int I, int H,
                        float* d_in, float* dWih_f, float* dWhh_f, float* dbih_f, float* dbhh_f, float* dWih_r,
                        float* dWhh_r, float* dbih_r, float* dbhh_r, float* workspace, void* stream);
int blvm_lstm_bidir_applies(int T, int B, int H);
int blvm_lstm_bidir_path_counts(unsigned long long out[2]);

/* ---------------------------------------------------------------------------------------------------------------
 * K2  single-layer GRU over a sequence (forward + BPTT), optionally time-reversed PER ROW.  Replaces `nn.GRU` and
 *     the `reverse_sequences` gathers around it, `blvm/models/srnn.py:113-116,196,200-206` +
 *     `blvm/utils/operations.py:56-87`: with reverse != 0 row b consumes time index lens[b]-1-j at recurrence step
 *     j < lens[b] and index j in its right padding, and its outputs are written back at those time indices.
 *     Gate rows [r|z|n] (torch.nn.GRU).
 *   in [T,B,I] with row stride ld_in; h0 [B,R] or NULL; out element (t,b,c) at out + t*out_ts + b*out_ld + c, so the
 *   states can be written straight into a wider time-major buffer; hn [B,R] state after the last recurrence step.
 * ------------------------------------------------------------------------------------------------------------- */
size_t blvm_gru_reserve_floats(int T, int B, int R);
size_t blvm_gru_bwd_workspace_floats(int T, int B, int R);
int blvm_gru_seq_fwd(const float* Wih, const float* Whh, const float* bih, const float* bhh, const float* in,
                     int ld_in, const float* h0, const int32_t* lens, int reverse, int T, int B, int I, int R,
                     float* out, long long out_ts, int out_ld, float* hn, float* reserve, void* stream);
/*   d_out addressed like out.  d_in [T,B,I] row stride ld_din (=|+= by accumulate_din), d_h0 [B,R]; weight grads
 *   ACCUMULATED; any output may be NULL. */
int blvm_gru_seq_bwd(const float* Wih, const float* Whh, const float* in, int ld_in, const int32_t* lens, int reverse,
                     const float* reserve, const float* d_out, long long out_ts, int out_ld, int T, int B, int I,
                     int R, float* d_in, int ld_din, int accumulate_din, float* d_h0, float* dWih, float* dWhh,
                     float* dbih, float* dbhh, float* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * K3  SRNN latent chain over a sequence (forward + BPTT).  Replaces the Python loop `blvm/models/srnn.py:224-253`
 *     (prior / posterior MLPs `srnn.py:92-111` on cat[d_t, z_{t-1}] / cat[a_t, z_{t-1}], residual posterior, rsample)
 *     and its autograd backward; the non-gated ("Elman") stochastic transfer that SRNNAudio builds.
 *   d, a [Tp,B,R]: deterministic forward state (shifted) and smoothing state; eps [Tp,B,Z]; z0 [B,Z] or NULL.
 *   zs [Tp+1,B,Z]: row 0 = z0, row t+1 = z_t.  slope: LeakyReLU slope of the MLPs (0.01).
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct BlvmSrnnWeights {
  const float *prior_w[3], *prior_b[3]; /* [H,R+Z] (input order cat[d,z]), [H,H], [H,H] */
  const float *prior_hw, *prior_hb;     /* [2Z,H] */
  const float *post_w[3], *post_b[3];   /* [H,R+Z] (input order cat[a,z]), [H,H], [H,H] */
  const float *post_hw, *post_hb;       /* [2Z,H] */
} BlvmSrnnWeights;

typedef struct BlvmSrnnGrads { /* same shapes; ACCUMULATED into (caller zeroes) */
  float *prior_w[3], *prior_b[3], *prior_hw, *prior_hb;
  float *post_w[3], *post_b[3], *post_hw, *post_hb;
} BlvmSrnnGrads;

size_t blvm_srnn_reserve_floats(int Tp, int B, int H, int Z, int R);
size_t blvm_srnn_bwd_workspace_floats(int Tp, int B, int H, int Z, int R);
int blvm_srnn_latent_fwd(const BlvmSrnnWeights* w, const float* d, const float* a, const float* z0, const float* eps,
                         int Tp, int B, int H, int Z, int R, int residual_posterior, float sd_eps, float slope,
                         float* zs, float* mu_q, float* sd_q, float* mu_p, float* sd_p, float* reserve, void* stream);
/*   d_z [Tp,B,Z]: gradient wrt z_t from outside the chain (the decoder).  KL folded in as for blvm_vrnn_seq_bwd.
 *   Outputs d_d, d_a [Tp,B,R], d_z0 [B,Z] (each may be NULL); grads accumulated. */
int blvm_srnn_latent_bwd(const BlvmSrnnWeights* w, const float* d, const float* a, const float* eps, const float* zs,
                         const float* mu_q, const float* sd_q, const float* mu_p, const float* sd_p,
                         const float* reserve, const float* d_z, const int32_t* x_sl, const float* c_raw,
                         const float* c_fn, int stride, float fn_floor, int Tp, int B, int H, int Z, int R,
                         int residual_posterior, float sd_eps, float slope, float* d_d, float* d_a, float* d_z0,
                         const BlvmSrnnGrads* grads, float* workspace, void* stream);

/* K3c  Ancestral sampling from SRNNAudio: every step of every utterance in ONE persistent launch (B <= 128).  Replaces the loop of
 *   `SRNN.generate` (`blvm/models/srnn.py:304-403`): enc = encoder(x_t) -> d_t = GRU(enc, d_{t-1}) -> prior(cat[d_t, z_{t-1}]) ->
 *   z_t = mu + sd eps -> decoder(cat[z_t, d_t]) -> DMoL head per sample -> draw -> x_{t+1}; 13 links per step dealt over all CUs
 *   (csrc/pchain.hip).  Weights in their PyTorch layouts; encoder / decoder are 3 x (Linear + LeakyReLU(slope)) as in
 *   `srnn.py:456-474`, x_dim = H.  x0 [B,S]; d0 [B,R], z0 [B,Z] or NULL (zeros); eps [T,B,Z]; u [T,B,S,num_mix], v [T,B,S] as in
 *   blvm_mix_sample (both NULL: the mode).  Outputs: x_out [B,T,S]; d_out [B,R] = d_T and z_out [T,B,Z] (each may be NULL).
 *   H, Z, R multiples of 16, num_mix = 10, any S >= 1 (padded inside the scratch as described at blvm_vrnn_generate).
 *   scratch: blvm_srnn_generate_scratch_floats(...) floats (weight copies + one slab per step of every activation). */
typedef struct BlvmSrnnDecodeWeights {
  const float *enc_w[3], *enc_b[3];                    /* [H,S], [H,H], [H,H] */
  const float *gru_wih, *gru_whh, *gru_bih, *gru_bhh;  /* d_forward_recurrent: [3R,H], [3R,R], [3R], [3R] */
  const BlvmSrnnWeights* chain;                        /* prior_* are read */
  const float *dec_w[3], *dec_b[3];                    /* [H,Z+R] (input order cat[z, d]), [H,H], [S*3*num_mix,H] */
  const float *lik_w, *lik_b;                          /* [3*num_mix, 3*num_mix], [3*num_mix] */
} BlvmSrnnDecodeWeights;
size_t blvm_srnn_generate_scratch_floats(int T, int B, int S, int H, int Z, int R);
int blvm_srnn_generate(const BlvmSrnnDecodeWeights* w, const float* x0, const float* d0, const float* z0, const float* eps,
                       const float* u, const float* v, int T, int B, int S, int H, int Z, int R, int num_mix, float sd_eps,
                       float slope, float log_eps, float* x_out, float* d_out, float* z_out, float* scratch, void* stream);
/* K3c with a head (the five scalars described at blvm_vrnn_generate_head: all three kinds, the same refusals before any launch or
 * write): blvm_srnn_generate is the kind-0 case (0, num_mix, log_eps, 0, 0).  The same arguments and layouts with the head in place
 * of `num_mix, log_eps`; dec_w[2] [S*F,H], lik_w [F,F], lik_b [F]; the scratch depends on F (0 for a kind that is not drawn).
 * Caller-owned buffers: results do not depend on the prior contents of scratch or of the outputs; nothing else is written. */
size_t blvm_srnn_generate_scratch_floats_head(int T, int B, int S, int H, int Z, int R, int head_kind);
int blvm_srnn_generate_head(const BlvmSrnnDecodeWeights* w, const float* x0, const float* d0, const float* z0, const float* eps,
                            const float* u, const float* v, int T, int B, int S, int H, int Z, int R, int head_kind, int num_mix,
                            float log_eps, float head_sd_beta, float head_sd_eps, float sd_eps, float slope, float* x_out,
                            float* d_out, float* z_out, float* scratch, void* stream);

/* K4c  Sampling from LSTMAudio: every step of every utterance in ONE persistent launch (B <= 128).  The loop of `LSTMAudio.generate`
 *   (`blvm/models/lstm.py`): emb = embedding(x_{t-1}) -> per layer (h, c) = LSTM cell(input, (h, c)) -> decoder(h of the last layer) ->
 *   DMoL head per sample -> draw -> x_t; 6 + 2 * num_layers links per step dealt over all CUs (csrc/lstm_decode.h).  Weights in
 *   their PyTorch layouts; embedding / decoder are 3 x (Linear + ReLU), the LSTM's input size is H; wih, whh, bih, bhh are HOST arrays
 *   of num_layers device pointers.  x0 [B,S] or NULL (zeros); h0, c0 [num_layers,B,H] or NULL (zeros); u [T,B,S,num_mix], v [T,B,S]
 *   as in blvm_mix_sample (both NULL: the mode).  Outputs: x_out [B,T,S]; h_out, c_out [num_layers,B,H] = the state after step T
 *   (each may be NULL).  H a multiple of 16, any S >= 1 through blvm_lstm_generate_any_stack (padded inside the scratch as described at
 *   blvm_vrnn_generate; blvm_lstm_generate keeps its published rule, S % 16 == 0, and is otherwise the same call), num_mix = 10,
 *   1 <= num_layers <= 8; T = 0 returns at once.
 *   scratch: blvm_lstm_generate_scratch_floats(...) floats (weight copies + one slab per step of every activation); results do not
 *   depend on what scratch or the outputs held before the call. */
typedef struct BlvmLstmDecodeWeights {
  const float *emb_w[3], *emb_b[3];                     /* [H,S], [H,H], [H,H] */
  const float *const *wih, *const *whh, *const *bih, *const *bhh; /* num_layers pointers each: [4H,H], [4H,H], [4H], [4H] */
  const float *dec_w[3], *dec_b[3];                     /* [H,H], [H,H], [S*3*num_mix,H] */
  const float *lik_w, *lik_b;                           /* [3*num_mix, 3*num_mix], [3*num_mix] */
} BlvmLstmDecodeWeights;
size_t blvm_lstm_generate_scratch_floats(int T, int B, int S, int H, int num_layers);
int blvm_lstm_generate_any_stack(const BlvmLstmDecodeWeights* w, const float* x0, const float* h0, const float* c0, const float* u,
                                 const float* v, int T, int B, int S, int H, int num_layers, int num_mix, float log_eps, float* x_out,
                                 float* h_out, float* c_out, float* scratch, void* stream);
/* The same call restricted to S % 16 == 0, as first published: any other S is refused before anything is touched. */
int blvm_lstm_generate(const BlvmLstmDecodeWeights* w, const float* x0, const float* h0, const float* c0, const float* u,
                       const float* v, int T, int B, int S, int H, int num_layers, int num_mix, float log_eps, float* x_out,
                       float* h_out, float* c_out, float* scratch, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * K10  WaveNet: dilated causal convolution (kernel size 2) and the gated residual block.  Replaces
 *      `CausalConv1d` (`blvm/models/wavenet/wavenet_modules.py:14-50`) and `Conv1dResidualGLU` (`:53-117`).
 *      Activations are TIME-MAJOR channel-last [L, B, C]; weights keep the Conv1d layout [C_out, C_in, k].
 *      out[t] = W[:,:,0] x[t] + W[:,:,1] x[t+dilation] + bias for t in [0, L_in - dilation)  (no padding: a block
 *      consumes `dilation` frames on the left, as the reference's stack does).
 * ------------------------------------------------------------------------------------------------------------- */
int blvm_scale_act_f32(const float* x, float scale, float slope, float* y, size_t n, void* stream); /* y = act(scale x) */
size_t blvm_conv1d_k2_workspace_floats(int Cin, int Cout);
int blvm_conv1d_k2_fwd(const float* x, const float* W, const float* bias, int L_in, int B, int Cin, int Cout,
                       int dilation, float* out, float* workspace, void* stream);
/*   d_x [L_in,B,Cin] (=), dW [Cout,Cin,2] (+=), db [Cout] (+=); each may be NULL. */
int blvm_conv1d_k2_bwd(const float* x, const float* W, const float* d_out, int L_in, int B, int Cin, int Cout,
                       int dilation, float* d_x, float* dW, float* db, float* workspace, void* stream);

/*   x [L_in,B,C]; conv_w [2C,C,2], conv_b [2C]; rs_w [C+S,C] (the 1x1 conv: first C rows residual, last S rows skip),
 *   rs_b [C+S]; o [L_in-dilation,B,C] = (res + x[dilation:]) * inv_std (may be NULL for the last block);
 *   skip [T_skip,B,S] += the last T_skip frames of the skip branch; S == 0 (skip NULL, rs_w = the first C rows): a block
 *   whose skip output is unused (STCN reads only every n-th block's skip, `stcn.py:301`).  reserve keeps pre-activations. */
size_t blvm_wavenet_block_reserve_floats(int L_in, int B, int C, int dilation);
size_t blvm_wavenet_block_workspace_floats(int L_in, int B, int C, int S, int dilation);
int blvm_wavenet_block_fwd(const float* x, const float* conv_w, const float* conv_b, const float* rs_w,
                           const float* rs_b, int L_in, int B, int C, int S, int dilation, int T_skip, float inv_std,
                           float* o, float* skip, float* reserve, float* workspace, void* stream);
/*   d_o may be NULL (last block); d_x [L_in,B,C] (=); weight grads (+=), each may be NULL. */
int blvm_wavenet_block_bwd(const float* x, const float* conv_w, const float* rs_w, const float* reserve,
                           const float* d_o, const float* d_skip, int L_in, int B, int C, int S, int dilation,
                           int T_skip, float inv_std, float* d_x, float* dconv_w, float* dconv_b, float* drs_w,
                           float* drs_b, float* workspace, void* stream);

/*   The whole residual stack in one call (`ResidualStack.forward`, `blvm/models/wavenet/wavenet_modules.py:178-215`: the loop over
 *   `Conv1dResidualGLU` blocks and the sum of their skip outputs): the host loop over blvm_wavenet_block_fwd / _bwd inside the library.
 *   params: HOST array of 4 n_blocks device pointers (conv_w, conv_b, rs_w, rs_b per block); dilations, groups: HOST arrays
 *   [n_blocks]; groups[i] = index into skips / d_skips of the tensor block i's skip branch is accumulated into, -1 = unused
 *   (that block runs with S = 0).  acts: the residual outputs of blocks 0 .. n-2 back to back, reserve: the blocks' reserves back
 *   to back (sizes from blvm_wavenet_stack_floats).  Backward: d_x [L,B,C] (=), d_scratch [L,B,C] (overwritten), grads: HOST array
 *   of 4 n_blocks device pointers (+=, each may be NULL). */
int blvm_wavenet_stack_floats(int L, int B, int C, const int* dilations, int n_blocks, size_t* acts_floats, size_t* reserve_floats);
int blvm_wavenet_stack_fwd(const float* x, const float* const* params, const int* dilations, const int* groups, int n_blocks, int L,
                           int B, int C, int S, int T_skip, float inv_std, float* acts, float* const* skips, float* reserve,
                           float* workspace, void* stream);
int blvm_wavenet_stack_bwd(const float* x, const float* const* params, const int* dilations, const int* groups, int n_blocks, int L,
                           int B, int C, int S, int T_skip, float inv_std, const float* acts, const float* reserve,
                           const float* const* d_skips, float* d_x, float* d_scratch, float* const* grads, float* workspace,
                           void* stream);

/* K10c  Autoregressive WaveNet sampling: all frames of all utterances in ONE launch, from an all-zero start.  Replaces the
 *   per-frame loop of `WaveNet.generate` (`blvm/models/wavenet/wavenet.py:254-293`) with the cached formulation its TODO
 *   names: block i keeps a ring buffer of its input over the last dilation_i frames.  in_channels = n_stack_frames = 1.
 *   packed: one weight image of blvm_wavenet_decode_pack_floats(C,S,O,n_blocks) floats, in this order (row-major,
 *     PyTorch parameter layouts): causal conv w [C,1,2], b [C]; in_transform w [C,C], b [C]; per block conv w [2C,C,2],
 *     b [2C], rs w [C+S,C], b [C+S]; out_transform Linear w [O,S], b [O]; head Linear w zero-padded to [32,O], b to [32].
 *   dilations: HOST array [n_blocks], n_blocks <= 64.  C, S, O multiples of 16; 3*num_mix <= 32.
 *   Per frame: skip sum * skip_scale -> ReLU -> Linear -> ReLU -> head Linear -> (logits, locs, log_scales) -> Gumbel-max
 *   component pick with u [n_frames,B,num_mix], logistic draw with v [n_frames,B] clamped to [-1,1] (as blvm_mix_sample
 *   kind 0; u = v = NULL: the mode) -> x_out [B,n_frames], fed back as the next input.
 *   scratch: blvm_wavenet_decode_scratch_floats(...) floats (ring buffers + operand-layout copies of the block weights;
 *   contents need no initialisation). */
size_t blvm_wavenet_decode_pack_floats(int C, int S, int O, int n_blocks);
size_t blvm_wavenet_decode_scratch_floats(const int* dilations, int n_blocks, int B, int C, int S);
int blvm_wavenet_decode(const float* packed, const int* dilations, int n_blocks, int B, int C, int S, int O, int num_mix,
                        int n_frames, float inv_std, float skip_scale, float log_eps, const float* u, const float* v,
                        float* scratch, float* x_out, void* stream);

/* K10c  The same sampling from a given state: continuing a prompt, or an earlier call (generation in chunks).
 *   The state after absolute frame t0 - 1 is (a) the ring buffers in scratch: block i's input over frames t0 - dilation_i ..
 *   t0 - 1 as [dilation_i,B,C], frame tau in slot tau mod dilation_i, block after block from float offset
 *   blvm_wavenet_decode_ring_offset_floats(n_blocks,C,S) = n_blocks ((2C)^2 + (C+S) C) of scratch, and (b) the last two
 *   samples x_in [B,2] = (previous, newest).  Frame tau of block 0's input is in_transform(causal conv of samples tau-2, tau-1).
 *   blvm_wavenet_decode_ring_fill: h [L,B,C] time-major, a block's input whose LAST frame is absolute frame t0 - 1
 *     (L >= dilation, t0 >= dilation; C a multiple of 4) -> its last `dilation` frames into ring [dilation,B,C]; every slot written.
 *   blvm_wavenet_decode_resume: arguments as blvm_wavenet_decode; no steady-state fill, frame t of the call is absolute frame
 *     t0 + t (t0 >= 0; only t0 mod dilation_i matters), u / v are indexed from 0 for the call.  The weight copies at the
 *     head of scratch are rewritten on every call (the weights may change between calls, the shapes may not); the ring region
 *     is read and updated in place.  x_state [B,2] (=): the sample pair after the last frame (may be x_in itself); with
 *     scratch it is the state after t0 + n_frames frames.  After blvm_wavenet_decode (t0 = 0) the rings in its scratch are
 *     that state too, with x_in = the last two columns of x_out (zeros in front of frame 0). */
size_t blvm_wavenet_decode_ring_offset_floats(int n_blocks, int C, int S);
int blvm_wavenet_decode_ring_fill(const float* h, int L, int B, int C, int dilation, int t0, float* ring, void* stream);
int blvm_wavenet_decode_resume(const float* packed, const int* dilations, int n_blocks, int B, int C, int S, int O, int num_mix,
                               int n_frames, int t0, float inv_std, float skip_scale, float log_eps, const float* u,
                               const float* v, const float* x_in, float* scratch, float* x_out, float* x_state, void* stream);

/* K10c  The same one-launch sampling with the categorical head (the softmax over V classes of K7d), from an all-zero start and from
 *   a state.  Arguments as for the DMoL pair above, except:
 *   V, levels, u replace num_mix, log_eps, u, v.  16 <= V <= 1024, V a multiple of 16 (anything else: BLVM_ENOSUP before any
 *     launch).  The packed image ends in the head Linear w [V,O], b [V] (no padding): blvm_wavenet_cat_decode_pack_floats floats.
 *     levels [V]: the value of class k — it is fed back as the next input and written to x_out as it stands (no arithmetic).
 *     u [n_frames,B]: one uniform draw per frame and row, or NULL.
 *   Per frame: ... -> head Linear -> logits l [V] -> NULL u: the arg-max class, first maximum; else the inverse CDF of
 *     e = exp(l - max l): the first class whose prefix sum reaches u * total, class V - 1 if none does.  The order of the sums is
 *     fixed: two calls on the same inputs agree to the bit.
 *   k_out [B,n_frames] int32 (=): the classes, or NULL.  x_out [B,n_frames] = levels[k].
 *   scratch, the rings, blvm_wavenet_decode_ring_fill, x_in / x_state: shared with the DMoL pair unchanged, so a state primed for
 *     one head serves the other. */
size_t blvm_wavenet_cat_decode_pack_floats(int C, int S, int O, int n_blocks, int V);
int blvm_wavenet_cat_decode(const float* packed, const int* dilations, int n_blocks, int B, int C, int S, int O, int V, int n_frames,
                            float inv_std, float skip_scale, const float* levels, const float* u, float* scratch, float* x_out,
                            int32_t* k_out, void* stream);
int blvm_wavenet_cat_decode_resume(const float* packed, const int* dilations, int n_blocks, int B, int C, int S, int O, int V,
                                   int n_frames, int t0, float inv_std, float skip_scale, const float* levels, const float* u,
                                   const float* x_in, float* scratch, float* x_out, int32_t* k_out, float* x_state, void* stream);

/* K10c  The same one-launch sampling with the Gaussian heads, from an all-zero start and from a state.  Arguments as for the DMoL
 *   pair above, except: head_kind, num_mix, sd_beta, sd_eps, u, n replace num_mix, log_eps, u, v.
 *   head_kind 1: the diagonal Gaussian mixture.  The head Linear is [3 num_mix, O] -> (logits, means, raw sds), zero-padded to [32,O]
 *     as the DMoL head's (3 num_mix <= 32).  Gumbel-max component pick with u [n_frames,B,num_mix], then x = mu + (softplus_beta(raw)
 *     + sd_eps) n with n [n_frames,B] standard normals (as blvm_mix_sample kind 1).  u and n are given together; both NULL: the
 *     arg-max component's mean.
 *   head_kind 2: the diagonal Gaussian.  The head Linear is [2,O] -> (mu, raw), zero-padded to [32,O]; num_mix is ignored, u must be
 *     NULL; x = mu + (softplus_beta(raw) + sd_eps) n, n NULL: the mean.
 *   Neither draw is clamped.  Any other head_kind, sd_beta <= 0 or sd_eps < 0: an error before any launch.
 *   packed: blvm_wavenet_decode_pack_floats floats.  scratch, the rings, blvm_wavenet_decode_ring_fill, x_in / x_state: shared with
 *     the DMoL pair unchanged. */
int blvm_wavenet_gauss_decode(const float* packed, const int* dilations, int n_blocks, int B, int C, int S, int O, int head_kind,
                              int num_mix, int n_frames, float inv_std, float skip_scale, float sd_beta, float sd_eps, const float* u,
                              const float* n, float* scratch, float* x_out, void* stream);
int blvm_wavenet_gauss_decode_resume(const float* packed, const int* dilations, int n_blocks, int B, int C, int S, int O, int head_kind,
                                     int num_mix, int n_frames, int t0, float inv_std, float skip_scale, float sd_beta, float sd_eps,
                                     const float* u, const float* n, const float* x_in, float* scratch, float* x_out, float* x_state,
                                     void* stream);

/* K10e  WaveNet with embedded class input (`WaveNet(embedding_dim=E, num_bins=V)`, `blvm/models/wavenet/wavenet.py:105-113,182`):
 *   nn.Embedding(V, E) and the causal convolution with groups = C, kernel size 2 (m = E / C inputs per output channel) as two lookup
 *   tables.  emb [V,E], cw [C,m,2], bias [C]; C a multiple of 4, C <= 1024.
 *   blvm_wavenet_embed_tables: P [2,V+1,C] (=), P[tap][k][o] = sum_j cw[o,j,tap] emb[k, o m + j] in index order; row V is zeros.
 *   blvm_wavenet_embed_fwd: k [L_in,B] int32 time-major classes, any value outside [0,V) (-1 by convention) a zero-padded frame ->
 *     out [L_out,B,C] (=), out[t,b] = (P[0][k[t,b]] + P[1][k[t+1,b]]) + bias, L_out = L_in - 1 - pad_causal (pad_causal: the last
 *     input is dropped, as in `CausalConv1d.forward`).
 *   blvm_wavenet_embed_bwd: d_out [L_out,B,C]; the caller sorts the n = (L_out + 1) B flattened classes of k[:L_out + 1] (padding
 *     mapped to V) with a stable sort: sorted_keys [n] ascending, perm [n] = the frame index tau B + b of every sorted entry,
 *     starts [V+1] = the first sorted position with a key >= k.  -> G [2,V,C] (=) the per-class sums of d_out by tap (an exact zero
 *     for a class without frames), d_emb [V,E] (=), d_cw [C,m,2] (=), d_bias [C] (=).  No float atomics: two calls agree to the bit.
 *     workspace: blvm_wavenet_embed_bwd_workspace_floats(n, V, C, m) floats (contents need no initialisation). */
int blvm_wavenet_embed_tables(const float* emb, const float* cw, int V, int C, int m, float* P, void* stream);
int blvm_wavenet_embed_fwd(const float* P, const float* bias, const int32_t* k, int L_in, int B, int V, int C, int pad_causal,
                           float* out, void* stream);
size_t blvm_wavenet_embed_bwd_workspace_floats(int n, int V, int C, int m);
int blvm_wavenet_embed_bwd(const float* d_out, const int32_t* sorted_keys, const int32_t* perm, const int32_t* starts, int L_out,
                           int B, int V, int C, int m, const float* emb, const float* cw, float* G, float* workspace, float* d_emb,
                           float* d_cw, float* d_bias, void* stream);

/* K10c  on the embedded model: the categorical pair above with the class fed back as a class.  tables = P [2,V+1,C] of
 *   blvm_wavenet_embed_tables replaces the causal convolution's weights (that region of the packed image is not read; its bias is):
 *   frame input = (P[0][k_prev] + P[1][k_new]) + bias.  The zero start is a past of class 0 (the reference's `embedding(zeros)`
 *   window, `wavenet.py:264-266`).  k_in / k_state [B,2] int32: the (previous, newest) class in place of x_in / x_state. */
int blvm_wavenet_embed_cat_decode(const float* packed, const float* tables, const int* dilations, int n_blocks, int B, int C, int S,
                                  int O, int V, int n_frames, float inv_std, float skip_scale, const float* levels, const float* u,
                                  float* scratch, float* x_out, int32_t* k_out, void* stream);
int blvm_wavenet_embed_cat_decode_resume(const float* packed, const float* tables, const int* dilations, int n_blocks, int B, int C,
                                         int S, int O, int V, int n_frames, int t0, float inv_std, float skip_scale,
                                         const float* levels, const float* u, const int32_t* k_in, float* scratch, float* x_out,
                                         int32_t* k_out, int32_t* k_state, void* stream);

/* K10d  Ancestral sampling from the STCN: all T steps of all rows in ONE launch, from an all-zero past.  The reference leaves
 *   `STCN.generate` unimplemented (`blvm/models/stcn/stcn.py:435-442`); this is the generative model its `forward` / `infer` define
 *   (`stcn.py:299-326, 389-409`) with every latent drawn from its prior.  Per step t: causal conv (kernel 2) of the stacks x_{t-2},
 *   x_{t-1} -> 1x1 in_transform -> n_blocks gated blocks (ring buffers as K10c), the skip half of block i read by level groups[i]
 *   (-1: by none; every level reads exactly one block: `d[n-1::n]` of `stcn.py:299`) -> for i = 0 .. n_latents-1, l = order[i]:
 *   (mu, sd) = prior[l](cat[skip_l, z[order[i-1]]]) (two 3-layer LeakyReLU MLPs of width C, sd = softplus_beta(.) + sd_eps,
 *   `stcn.py:32-76`), z[l] = mu + sd * eps[l][t] -> the output stack (1x1 in_transform on cat(z) if dense else z[0], n_out gated
 *   blocks of dilation 1, skips summed; its past before step 0 is the response to `forward`'s zero padding, `stcn.py:389-395`)
 *   -> * out_scale -> out_upsample Linear + ReLU -> [S, 3 num_mix] -> head Linear per sample -> draw as blvm_mix_sample kind 0 with
 *   u [T,B,S,num_mix], v [T,B,S] (both NULL: the mode) -> x_out [B,T,S], fed back.
 *   packed: one image of blvm_stcn_generate_pack_floats(...) floats, row-major PyTorch layouts, in this order: causal conv w [C,S,2],
 *     b [C]; in_transform w [C,C], b [C]; per block conv w [2C,C,2], b [2C], rs w [2C,C], b [2C]; per level l = 0 .. n-1 the mu then
 *     the sd MLP, each w0 [C,Kin_l] b0 [C] w1 [C,C] b1 [C] w2 [Z_l,C] b2 [Z_l] (Kin_l = C, + Z of the level visited before l unless l
 *     is visited first); output in_transform w [C,Zin], b [C]; per output block as above; out_upsample w and b zero-padded to the
 *     next multiple of 16 rows; head w zero-padded to [32,32], b to [32].
 *   dilations, groups [n_blocks], latent, order [n_latents]: HOST int arrays; eps, z_out, mu_out, sd_out: HOST arrays of n_latents
 *     device pointers, each [T,B,Z_l] (z_out, mu_out, sd_out: the draws and the prior parameters of every step).
 *   C and every Z_l multiples of 16; S >= 1 (any); 3 num_mix <= 32; n_latents <= 8; n_blocks, n_out <= 64; at most 160 KB
 *     of LDS — anything else is refused before a buffer is touched.
 *   scratch: blvm_stcn_generate_scratch_floats(...) floats (operand-layout weight copies, the blocks' rings, the selected skips);
 *     results do not depend on what scratch or the outputs held before the call. */
size_t blvm_stcn_generate_pack_floats(int C, int S, int n_blocks, int n_out, const int* latent, const int* order, int n_latents,
                                      int dense, int num_mix);
size_t blvm_stcn_generate_scratch_floats(const int* dilations, int C, int S, int n_blocks, int n_out, const int* latent,
                                         const int* order, int n_latents, int dense, int num_mix, int B);
int blvm_stcn_generate(const float* packed, const int* dilations, const int* groups, int n_blocks, int n_out, const int* latent,
                       const int* order, int n_latents, int dense, int B, int C, int S, int num_mix, int T, float inv_std,
                       float out_scale, float sd_beta, float sd_eps, float slope, float log_eps, const float* const* eps,
                       const float* u, const float* v, float* x_out, float* const* z_out, float* const* mu_out,
                       float* const* sd_out, float* scratch, void* stream);

/* K10d  The same sampling from a given state: continuing a prompt, or an earlier call (generation in chunks).
 *   The state after absolute step t0 - 1 is (a) the rings in scratch, from float offset
 *   blvm_stcn_generate_ring_offset_floats(...) (= the packed image's size; the operand copies lie below it): dilated block i's input
 *   over steps t0 - dilation_i .. t0 - 1 as [dilation_i,B,C], step tau in slot tau mod dilation_i, block after block; then output
 *   block j's input at step t0 - 1 as [B,C], j = 0 .. n_out-1; then the selected skips [n_latents,B,C], which are no state; and
 *   (b) the two newest stacks x_in [B,2,S] = (x_{t0-2}, x_{t0-1}).  Step tau of dilated block 0's input is in_transform(causal conv
 *   of the stacks x_{tau-2}, x_{tau-1}); of output block 0's, the output in_transform of cat(z_tau) (dense) or z_tau[0]; stacks and
 *   latents in front of step 0 are zero.  blvm_wavenet_decode_ring_fill (K10c) serves these rings too: they have its layout.
 *   blvm_stcn_generate_resume: arguments as blvm_stcn_generate; no steady-state fill, step t of the call is absolute step t0 + t
 *     (t0 >= 0; only t0 mod dilation_i matters; t0 + T < 2^31 - 1); eps, u, v and every output are indexed from 0 for the call.
 *     The operand copies at the head of scratch and the selected skips are rewritten on every call (the weights may change between
 *     calls, the shapes may not; results do not depend on what those regions or the outputs held); the ring region is read and
 *     updated in place.  x_state [B,2,S] (=): the two newest stacks after the last step (may be x_in itself); with scratch it is the
 *     state after t0 + T steps.  T = 0: x_in is copied to x_state on the stream and nothing else is launched.  Refuses whatever
 *     blvm_stcn_generate refuses, NULL x_in / x_state and t0 < 0 — before a buffer is touched.
 *   After blvm_stcn_generate the rings in its scratch are the state after T steps: t0 = T, x_in = the last two stacks of x_out (zero
 *     stacks in front of step 0). */
size_t blvm_stcn_generate_ring_offset_floats(int C, int S, int n_blocks, int n_out, const int* latent, const int* order,
                                             int n_latents, int dense, int num_mix);
int blvm_stcn_generate_resume(const float* packed, const int* dilations, const int* groups, int n_blocks, int n_out,
                              const int* latent, const int* order, int n_latents, int dense, int B, int C, int S, int num_mix,
                              int T, float inv_std, float out_scale, float sd_beta, float sd_eps, float slope, float log_eps,
                              const float* const* eps, const float* u, const float* v, float* x_out, float* const* z_out,
                              float* const* mu_out, float* const* sd_out, float* scratch, int t0, const float* x_in,
                              float* x_state, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * K5  RSSM cell of the Clockwork-VAE over a sequence (forward + BPTT).  Replaces the per-level time loop
 *     `blvm/models/clockwork_vae/clockwork_vae.py:272-281` over `RSSMCell.forward` (`blvm/modules/rssm.py:79-104`).
 *   enc [T,B,E] encodings of this level; ctx [T,B,C] context from the level above (C may be 0, ctx NULL);
 *   z0 [B,Z], h0 [B,H] or NULL (zeros); eps [T,B,Z];
 *   mode: 0 plain, 1 residual posterior (mu_q += mu_p), 2 precision-weighted posterior (`variational.py:125-138`).
 *   zs [T+1,B,Z], hs [T+1,B,H]: row 0 = initial state, row t+1 = state after step t (the context for the level below
 *   is cat[zs[1:], hs[1:]]).  mu_q/sd_q are the COMBINED posterior parameters the KL is taken against.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct BlvmRssmWeights {
  const float *gin_w, *gin_b;           /* [H, Z+C] (input order cat[z, context]), [H] */
  const float *gru_wih, *gru_whh;       /* [3H,H] each, rows [r|z|n] */
  const float *gru_bih, *gru_bhh;       /* [3H] */
  const float *prior_w[3], *prior_b[3]; /* [H,H] x3 */
  const float *prior_hw, *prior_hb;     /* [2Z,H] */
  const float *post_w[3], *post_b[3];   /* [H,H+E] (input order cat[h, enc]), [H,H], [H,H] */
  const float *post_hw, *post_hb;       /* [2Z,H] */
} BlvmRssmWeights;

typedef struct BlvmRssmGrads { /* same shapes; ACCUMULATED into (caller zeroes) */
  float *gin_w, *gin_b, *gru_wih, *gru_whh, *gru_bih, *gru_bhh;
  float *prior_w[3], *prior_b[3], *prior_hw, *prior_hb;
  float *post_w[3], *post_b[3], *post_hw, *post_hb;
} BlvmRssmGrads;

size_t blvm_rssm_reserve_floats(int T, int B, int H, int Z);
size_t blvm_rssm_bwd_workspace_floats(int T, int B, int H, int Z);
int blvm_rssm_seq_fwd(const BlvmRssmWeights* w, const float* enc, const float* ctx, const float* z0, const float* h0,
                      const float* eps, int T, int B, int H, int Z, int C, int E, int mode, float sd_eps, float* zs,
                      float* hs, float* mu_q, float* sd_q, float* mu_p, float* sd_p, float* reserve, void* stream);
/*   d_zs [T+1,B,Z], d_hs [T+1,B,H]: gradients wrt zs / hs from outside the chain (rows 1.. = the states, row 0 = the
 *   initial state).  KL folded in as for blvm_vrnn_seq_bwd (stride = level stride in audio frames).
 *   Outputs (each may be NULL): d_enc [T,B,E], d_ctx [T,B,C], d_z0 [B,Z] (complete), d_h0 [B,H] (WITHOUT d_hs[0]). */
int blvm_rssm_seq_bwd(const BlvmRssmWeights* w, const float* enc, const float* ctx, const float* eps, const float* zs,
                      const float* hs, const float* mu_q, const float* sd_q, const float* mu_p, const float* sd_p,
                      const float* reserve, const float* d_zs, const float* d_hs, const int32_t* x_sl,
                      const float* c_raw, const float* c_fn, int stride, float fn_floor, int T, int B, int H, int Z,
                      int C, int E, int mode, float sd_eps, float* d_enc, float* d_ctx, float* d_z0, float* d_h0,
                      const BlvmRssmGrads* grads, float* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * K11  Clockwork-VAE convolutional coders: the streaming pieces of `BlockSeparable`
 * (`blvm/models/clockwork_vae/convolutional_coders.py:29-66`), `ConvDepthwiseSeparable1d` /
 * `ConvTransposeDepthwiseSeparable1d` (`blvm/modules/convolutions.py:6-104`) and `TemporalResidual`
 * (`convolutional_coders.py:15-26`).  Layout: time-major channel-last [L,B,C] seen as a matrix [L, N=B*C]
 * (C a multiple of 4).  The block's 1x1 convolutions are blvm_gemm_f32 calls on [L*B, C].
 *
 * chan_norm: nn.GroupNorm(num_groups=C, C) == per-(sample,channel) normalisation over time, biased variance, eps;
 *   y = (x-mean)*rstd*gamma_c + beta_c;  mr [2,N] receives [mean | rstd] (kept for backward);
 *   workspace: blvm_chan_norm_workspace_doubles(N) float64.
 *   blvm_chan_norm_stats: statistics only — mr and the column affine scale_shift [2,N] = [rstd*gamma | beta - mean*rstd*gamma]
 *   for consumers that normalise on load (blvm_dwconv_*'s in_scale / in_shift), so the normalised tensor never hits HBM.
 *   bwd: dx (relu_mask=1 multiplies by (x>0): a ReLU feeding the norm), dgamma/dbeta ACCUMULATED (may be NULL),
 *   dx_chan_sum [C] (may be NULL) += sum over rows and samples of dx (the bias gradient of the layer that produced x).
 * dwconv: depthwise Conv1d (transposed=0: L_out=(L_in-k_eff)/stride+1) or ConvTranspose1d (transposed=1:
 *   L_out=(L_in-1)*stride+k_eff), k<=8, no padding (callers pad), weights [C,k] (= torch [C,1,k]), bias [C] or NULL,
 *   relu=1 fuses a ReLU on the output (bwd then needs y).  in_scale/in_shift ([N] each, or both NULL): the convolution
 *   runs on x*in_scale + in_shift (column-wise).  bwd: dx = gradient wrt that transformed input (may be NULL),
 *   dw/dbias ACCUMULATED (may be NULL).
 * resample_add: out[t] = y[t] + x[nearest(t)], nearest(t)=min(floor(t*float(L_in)/L_out), L_in-1) (F.interpolate
 *   mode='nearest');  bwd ACCUMULATES dout into dx [L_in,N] (dy is dout itself).
 * Every [L,N] tensor and every [N] / [2,N] / [C] vector that a kernel reads or writes four columns at a time must be
 *   16-byte aligned (resample_add_fwd's y, x and out and dwconv's in_scale / in_shift included): BLVM_EINVAL otherwise.
 * ------------------------------------------------------------------------------------------------------------- */
size_t blvm_chan_norm_workspace_doubles(int N);
int blvm_chan_norm_stats(const float* x, int L, int N, int C, const float* gamma, const float* beta, float eps, float* mr,
                         float* scale_shift, double* workspace, void* stream);
int blvm_chan_norm_fwd(const float* x, int L, int N, int C, const float* gamma, const float* beta, float eps, float* y,
                       float* mr, double* workspace, void* stream);
int blvm_chan_norm_bwd(const float* x, const float* dy, const float* mr, const float* gamma, int L, int N, int C,
                       int relu_mask, float* dx, float* dgamma, float* dbeta, float* dx_chan_sum, double* workspace,
                       void* stream);
int blvm_dwconv_out_length(int L_in, int k, int stride, int dilation, int transposed);
int blvm_dwconv_fwd(const float* x, const float* in_scale, const float* in_shift, const float* w, const float* bias,
                    int L_in, int N, int C, int k, int stride, int dilation, int transposed, int relu, float* y,
                    void* stream);
int blvm_dwconv_bwd(const float* x, const float* in_scale, const float* in_shift, const float* w, const float* y,
                    const float* dy, int L_in, int N, int C, int k, int stride, int dilation, int transposed, int relu,
                    float* dx, float* dw, float* dbias, void* stream);
int blvm_resample_add_fwd(const float* y, const float* x, int L_out, int L_in, int N, float* out, void* stream);
int blvm_resample_add_bwd(const float* dout, int L_out, int L_in, int N, float* dx, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * K9  CTC loss on UN-NORMALISED logits and the greedy CTC decode.  Replaces `logits.log_softmax(2)` + `nn.CTCLoss(blank,
 *     reduction="none")` and the host `greedy_ctc`, `blvm/models/lstm_asr.py:67-72` + `blvm/utils/decoding.py:5-29`.
 *   logits [T,B,C] time-major; targets [B,Lmax] int32, right-padded; input_lens, target_lens [B] int32 (device).
 *   nll [B]: -log p(targets[b,:target_lens[b]] | first input_lens[b] frames), +inf for a row with too few frames for its labels.
 *   d_logits [T,B,C] or NULL (loss only): d_nll[b] * (softmax_t(c) - occupation_t(c)) for t < input_lens[b], exactly 0 beyond;
 *   d_nll [B] is the upstream gradient, NULL = ones.  A row with nll = +inf has NaN gradients over its frames (torch's
 *   zero_infinity=False).  A label outside [0,C) or a length outside [0,T] / [0,Lmax] makes that row's nll and gradient NaN;
 *   such a value is never used as an index.  No atomics: results are bit-identical from call to call.
 *   Limits: T, B >= 1, T * B < 2^31, 2 <= C <= 4096, 0 <= Lmax <= 512, 0 <= blank < C.
 *   scratch: blvm_ctc_scratch_floats(T, B, C, Lmax) floats (the per-step log-sum-exp and alpha, beta [B,T,2 Lmax + 1]).
 * blvm_ctc_greedy: per row the arg-max of each of the first input_lens[b] frames (lowest index on a tie), repeats collapsed, blanks
 *   dropped: hyp [B,T] int32 holds hyp_lens[b] labels per row, -1 behind them.
 * ------------------------------------------------------------------------------------------------------------- */
size_t blvm_ctc_scratch_floats(int T, int B, int C, int Lmax);
int blvm_ctc_loss(const float* logits, const int32_t* targets, const int32_t* input_lens, const int32_t* target_lens, int T,
                  int B, int C, int Lmax, int blank, const float* d_nll, float* nll, float* d_logits, float* scratch,
                  void* stream);
int blvm_ctc_greedy(const float* logits, const int32_t* input_lens, int T, int B, int C, int blank, int32_t* hyp,
                    int32_t* hyp_lens, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * K9  Batched Levenshtein distance (unit-cost substitutions, insertions, deletions) between integer sequences, with an optional
 *     token -> unit expansion.  Replaces the host `edit_distance` of the error-rate metrics, `blvm/evaluation/metrics.py:68-85`.
 *   ref [B,ref_stride], hyp [B,hyp_stride] int32 with ref_len, hyp_len [B] int32 (device): only the first len entries of a row are
 *   read, whatever lies behind them (the -1 padding of blvm_ctc_greedy included).
 *   n_tables = 0: the sequences are compared as they are; unit_offsets, units, separators, V and max_units are ignored.
 *   n_tables >= 1: ONE launch serves every table over the same sequences (grid B x n_tables).  unit_offsets [n_tables,V + 1] are
 *   CSR offsets into the shared array `units`: under table k token v stands for units[unit_offsets[k][v] .. unit_offsets[k][v + 1]),
 *   possibly none; separators[k] >= 0 is inserted between every two consecutive tokens (not before the first, not after the
 *   last), < 0: no separator.  max_units: the longest unit list of any token (host side; it sizes the kernel's LDS).
 *   edits, ref_units [max(n_tables,1),B]: the distance between the expanded sequences and the expanded reference's length.  A token
 *   outside [0,V) inside a row's length (tables only) or a length outside [0,stride] makes edits = ref_units = -1 for that row and
 *   table alone; such a value is never used as an index.  totals [max(n_tables,1),3] or NULL: per table the sum of edits and of
 *   ref_units over the accepted rows and the number of refused rows, summed in a fixed order by a second small launch.
 *   No atomics; every element is written on every call: bit-identical from call to call, whatever the buffers held.
 *   Limits: an expanded reference row of at most 8192 units, judged by its bound ref_stride * (max_units + 1) - 1 (ref_stride
 *   without tables); hyp_stride * (max_units + 1) < 2^30 (any hypothesis length: it is walked in strips of 512 units);
 *   n_tables <= 65535.
 * ------------------------------------------------------------------------------------------------------------- */
int blvm_edit_distance(const int32_t* ref, const int32_t* ref_len, int ref_stride, const int32_t* hyp, const int32_t* hyp_len,
                       int hyp_stride, int B, int n_tables, int V, const int32_t* unit_offsets, const int32_t* units,
                       const int32_t* separators, int max_units, int32_t* edits, int32_t* ref_units, int32_t* totals, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * K10Log-mel spectrogram front end of the probe, on the device and per batch.  Replaces the loader-side
 *     `torchaudio.transforms.MelSpectrogram` (its defaults: centred frames, reflect padding, periodic Hann, power 2, HTK mel
 *     scale, no filter norm) + `10 log10(clamp_min(., 1e-10))` + per-bin mean / std, `blvm/data/transforms.py:113-166`.
 *   wave [B,Lmax] right-padded; lens [B] int32 (device): L_b valid samples, n_fft / 2 < L_b <= Lmax.  Frame t of row b is centred
 *   on sample t * hop_length; samples outside [0, L_b) are reflected about the row's OWN ends.  T_b = 1 + L_b / hop_length.
 *   basis [WP,2,NBP]: basis[n,0,k] = w[n] cos(2 pi k (left + n) / n_fft), basis[n,1,k] = the sine, w the periodic Hann window of
 *   win_length, left = (n_fft - win_length) / 2, k < n_bins = n_fft / 2 + 1; rows n >= win_length and columns k >= n_bins are 0.
 *   fbank [NBP,NMP]: the mel filters, zero-padded.  WP = win_length rounded up to 8; NBP, NMP = n_bins, n_mels rounded up to 32.
 *   out [B,n_mels,T_max], T_max = 1 + Lmax / hop_length: 10 log10(max(mel power, 1e-10)); with normalize = 1 every (b, mel) row
 *   then has its mean over its T_b frames subtracted and is divided by (unbiased standard deviation + 1e-10): a constant row comes
 *   out exactly 0, a row of one frame NaN (as torch.std).  Columns t >= T_b are written as 0 and out_lens[b] = T_b on every call;
 *   nothing depends on the buffers' earlier contents.  A row whose length is outside (n_fft / 2, Lmax] is NaN throughout with
 *   out_lens[b] = 0; such a length is never used as an index.  No atomics: bit-identical from call to call, and a row's result
 *   does not depend on the other rows of the batch.
 *   Limits: n_fft even, 16 <= win_length <= n_fft <= 1024, hop_length >= 1, 1 <= n_mels <= 128, Lmax > n_fft / 2,
 *   B * T_max < 2^31, B * n_mels < 2^31.
 * ------------------------------------------------------------------------------------------------------------- */
int blvm_logmel(const float* wave, const int32_t* lens, int B, int Lmax, int n_fft, int win_length, int hop_length, int n_mels,
                const float* basis, const float* fbank, int normalize, float* out, int32_t* out_lens, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BLVM_HIP_H */
