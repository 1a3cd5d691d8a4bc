/*
 * mmb.h — C ABI of libmmb.so, the MI355X (gfx950) SIF / MMB2 / regressor hot path.
 *
 * The reference (yaochie/multimodal-baselines) has no FFI: its boundary is a set
 * of Python functions on numpy arrays / torch tensors.  Each entry point below
 * replaces the arithmetic of one of those functions; the Python mirror in
 * `multimodal-baselines_amd/` keeps the reference names and signatures and
 * calls these through ctypes.
 *
 * Conventions:
 *   - every pointer argument except host_* is DEVICE memory allocated by the
 *     caller; the library never allocates or frees caller memory;
 *   - all work is enqueued on `stream` and is asynchronous; no entry point
 *     synchronises, so the calls can be captured into a hipGraph;
 *   - row-major, contiguous layouts; ids are int32 (the caller narrows the
 *     reference's int64 ids after a range check);
 *   - a pointer carries no element type: the Python mirrors state each
 *     operand's at the hand-over (mmb_lib.ptr(tensor, dtype): float -> float32,
 *     double -> float64, int32_t / uint32_t -> int32, int64_t -> int64,
 *     uint8_t -> uint8; a `void*` operand names the types it takes) and raise
 *     before anything is launched on a tensor of another type, a host tensor
 *     or a non-contiguous one (tests/test_presentation_cases.py reads the
 *     types off this header);
 *   - return 0 on success, MMB_EINVAL (<0) on a bad argument or shape, or a
 *     positive hipError_t from the launch;
 *   - `flag` (nullable) is an int32 device word OR-ed with MMB_FLAG_* bits by
 *     kernels that meet out-of-range ids (the shim raises IndexError, like
 *     numpy would in the reference) or all-zero-weight utterances (the shim
 *     raises ValueError where the reference's PC step would).
 *
 * Scratch and outputs on entry: what a caller-owned workspace (`ws`,
 * `colmax_ws`, `dh_ws`), an output buffer or a derived image (wm, c0, wsplit,
 * wpieces, the text cache, the normalised word table) holds when a call
 * starts is unspecified, and no output depends on it: every slot a kernel
 * reads was written by this call (or by the builder of the image, which
 * writes every byte its *_bytes query counts, pads included; the one gap is
 * described at mmb_mm2_text_cache), and a pad documented as zero is written
 * as zero.  The exceptions are stated at their
 * entry points and are all words that workgroups synchronise on, which must
 * be zero on entry and are left zero: the first 16 bytes of mmb_pc_solve_mc's
 * ws and the whole ws of mmb_mlp_train (mmb_mm2_stream_project zeroes its
 * counter at the end of colmax_ws itself).  An output that `accumulate` adds
 * to is an input.  tests/test_gpu_scratch.py holds every entry point to this
 * with three byte patterns.
 */
#ifndef MMB_H_
#define MMB_H_

#include <stdint.h>
#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMB_OK 0
#define MMB_EINVAL (-1)
#define MMB_FLAG_ID_RANGE 1
/* an utterance whose SIF weights are all 0 (its a2 row is 0/0 = NaN, like
 * numpy's; the reference's TruncatedSVD then raises ValueError on the split) */
#define MMB_FLAG_ZERO_WEIGHTS 2
/* mmb_mm2_stream_project: a hand-over between its streaming and projecting
 * waves waited ~0.5 s without progress (a bug, never expected); the kernel
 * then ends at once and its MMB2 rows are invalid */
#define MMB_FLAG_SYNC_TIMEOUT 4

/* Library version (major*10000 + minor*100 + patch). */
int mmb_version(void);

/* ---------------------------------------------------------------- a1
 * seq2weight: w[i,j] = f32(wtab64[seq[i,j]]) if sel[i,j] (nullable = all) and
 * seq[i,j] >= 0, else 0.  Bit-exact with the reference.
 * replaces: sif_functions.seq2weight   /root/reference/sif_functions.py:8-15
 *           sif.get_sentence_word_weights /root/reference/sif.py:78-82      */
int mmb_seq2weight(const int32_t* seq, const uint8_t* sel, int64_t n, int64_t l,
                   const double* wtab64, int64_t v, float* w_out, int32_t* flag,
                   hipStream_t stream);

/* ---------------------------------------------------------------- a1+a2
 * Weighted average of gathered table rows per utterance:
 *   num[i] = sum_j w[i,j] * table[ids[i,j]],  cnt[i] = count_nonzero(w[i,:]),
 *   x[i]   = num[i] / cnt[i]                       (all float32)
 * Weights come from `w` [n,l] when non-null (get_weighted_average), else from
 * the f32 table `wtab32` gathered by id with id<0 -> 0 (a1 fused).
 * Negative ids wrap like numpy (table[v+id]).  Outputs x/num/cnt are each
 * nullable (at least one required).
 * replaces: sif_functions.get_weighted_average /root/reference/sif_functions.py:28-56 */
int mmb_sif_wavg(const float* table, int64_t v, int d, const int32_t* ids, int64_t n, int l,
                 const float* w, const float* wtab32, float* x_out, float* num_out,
                 float* cnt_out, int32_t* flag, hipStream_t stream);

/* mmb_sif_wavg on a word table kept in 16-bit storage: table [v,d] contiguous
 * holds elements of table_type.  A table value is widened to f32 in registers
 * right after its (plain, cached: the rows are the reused data) load -- exact
 * for both 16-bit types, fp16 subnormals included -- and summed by the
 * statements of mmb_sif_wavg in their order, the workgroup kernel's row-0
 * shortcut (w0 E0 entering once) included: x, num and cnt are bit for bit
 * what mmb_sif_wavg writes for the same table upcast to f32 by the caller.
 * The library rounds nothing: the caller chose the 16-bit values.  Outputs,
 * the empty call and the flag bits are mmb_sif_wavg's.
 * MMB_TABLE_F32 is mmb_sif_wavg itself for the same arguments.
 * 16-bit table: the wave kernel at l <= 64, d % 4 == 0 and <= 512, table
 * 8-byte and x_out / num_out 16-byte aligned (a column unit is 4 values = one
 * 8-byte load); otherwise the workgroup kernel, in 4-value units when
 * d % 4 == 0 and the table is 8-byte aligned (d up to 1280), in scalar 2-byte
 * loads if not (d up to 320).
 * MMB_EINVAL before any launch: a table_type outside 0..2 (also with n == 0),
 * a 16-bit table that is not 2-byte aligned, null ids, anything mmb_sif_wavg
 * rejects.
 * replaces: sif_functions.get_weighted_average /root/reference/sif_functions.py:28-56
 *   (which reads an f32 table only)                                          */
#define MMB_TABLE_F32 0
#define MMB_TABLE_F16 1 /* IEEE binary16 */
#define MMB_TABLE_BF16 2
int mmb_sif_wavg_tt(const void* table, int table_type, int64_t v, int d, const int32_t* ids,
                    int64_t n, int l, const float* w, const float* wtab32, float* x_out,
                    float* num_out, float* cnt_out, int32_t* flag, hipStream_t stream);

/* ---------------------------------------------------------------- a3 (Gram)
 * g[d,d] (float64, full symmetric) = sum_i x_i x_i^T with x_i = num[i]/cnt[i]
 * (cnt nullable -> x = num).  Products of f32 values are exact in f64 (fp64
 * MFMA).  `ws` is scratch of mmb_gram_workspace_bytes(n, d) bytes.
 * If accumulate != 0 the result is added to g (multi-split use).            */
size_t mmb_gram_workspace_bytes(int64_t n, int d);
int mmb_gram(const float* num, const float* cnt, int64_t n, int d, double* g, int accumulate,
             void* ws, hipStream_t stream);

/* The same Gram in two phases, for a split streamed in row chunks (the
 * overlapped bench step): mmb_gram_part reduces one chunk of n <= n_plan rows
 * into per-range partials in ws (accumulate = 0 for the first chunk, 1 to add
 * the next ones; every chunk must use the same n_plan, and consecutive calls
 * must be stream-ordered); mmb_gram_finish sums the partials in a fixed order
 * into g (accumulate: add to g).  ws as for mmb_gram(n_plan, d); d % 4 == 0,
 * d <= 320, num 16-byte aligned.                                             */
int mmb_gram_part(const float* num, const float* cnt, int64_t n, int64_t n_plan, int d,
                  int accumulate, void* ws, hipStream_t stream);
int mmb_gram_finish(int64_t n_plan, int d, double* g, int accumulate, const void* ws,
                    hipStream_t stream);

/* The same Gram on the int8 matrix pipe, for x rows (cnt = 1) whose column
 * bounds colmax[j] = max_i |x[i,j]| (float bits) are known: every value as a
 * 30-bit fixed-point integer of its column's power-of-two bound, cut into
 * four int8 digits; digit-pair products of level <= 4 summed exactly (int32
 * per 64-row step, then f64).  Not bit-equal to mmb_gram: ~1e-10 relative
 * (the PC within 6e-11 of the reference's on the golden splits).  d % 4 == 0,
 * d <= 304; ws as for mmb_gram_workspace_bytes(n, d).  mmb_colmax computes
 * the bounds (accumulate = 0 zeroes colmax first).
 * replaces: the X^T X inside sif_functions.compute_pc's TruncatedSVD
 *   /root/reference/sif_functions.py:58-67                                   */
int mmb_colmax(const float* x, int64_t n, int d, uint32_t* colmax, int accumulate,
               hipStream_t stream);
int mmb_gram_i8(const float* x, const uint32_t* colmax, int64_t n, int d, double* g,
                int accumulate, void* ws, hipStream_t stream);

/* z0[d,k] = X^T omega  (omega [n,k] float64) — start block of the transposed
 * randomized-SVD branch (n < d).                                             */
int mmb_xt_omega(const float* num, const float* cnt, int64_t n, int d, const double* omega,
                 int k, double* z0, hipStream_t stream);

/* ---------------------------------------------------------------- a3 (solve)
 * Top-npc right singular vectors of X exactly as scikit-learn's
 * TruncatedSVD(npc, n_iter, random_state=0) (randomized_svd, k = npc+10
 * oversampled block, LU-normalised power iterations, svd_flip on components)
 * computes them, evaluated from the Gram g alone: span(G^n_iter Z0) is the
 * subspace the reference's iterations build, and the final SVD of Q^T X is
 * solved as a k x k (generalised) symmetric eigenproblem.  One workgroup, fp64.
 *   transposed = (n_total < d): z0 = X^T Omega_n, else z0 = Omega_d [d,k].
 * pc_out [npc, d] float64.  d <= 512, k <= min(16, d): a block wider than the
 * space has singular k x k factors and is rejected (MMB_EINVAL, as in the two
 * entry points below); its first d columns already span everything.
 * Accuracy (all three solve entry points; tests/test_gpu_spectrum.py): the
 * first component stays within 1e-12 of the reference's up to l1/l11 = 1e10
 * and down to l1/l2 - 1 = 1e-4 (1e-10 at 1e-6: eps / gap).  The solve sees X
 * only through G, so component c carries about eps * l1/lc whatever the
 * kernel does: 2e-12 at l1/l2 = 6e4, 1e-10 at 6e6, 2e-8 at 6e8 for the second
 * one (the CPU oracle's Gram route measures the same).  A caller who needs
 * later components beyond that on such a spectrum needs the rows, not G.
 * replaces: sif_functions.compute_pc /root/reference/sif_functions.py:58-67 */
int mmb_pc_solve(const double* g, int d, const double* z0, int k, int npc, int n_iter,
                 int transposed, double* pc_out, hipStream_t stream);

/* The same solve on ceil(d/16) workgroups (d <= 320, k <= min(16, d): a wider
 * block is rejected, MMB_EINVAL): each keeps
 * 16 rows of G in registers, the tiles of every power-iteration product are
 * exchanged in-launch (write-through stores + an arrival counter), and every
 * workgroup runs the identical CholeskyQR; workgroup 0 runs the final
 * Rayleigh-Ritz step.  ws: mmb_pc_solve_mc_ws_bytes(d) bytes, 16-byte
 * aligned, owned by the call until it completes; its first 16 bytes (arrival
 * counter, abort word) must be ZERO when the caller first hands it over, and
 * a completed solve leaves them zero -- no memset is enqueued, so the call is
 * safe to capture into a graph and replay.  A workgroup that waits ~1 s for
 * the others gives up and sets MMB_FLAG_SYNC_TIMEOUT in *flag (nullable);
 * so does a launch that finds the words dirty (an abort word left set, or an
 * arrival count outside the round's range); pc_out is then NaN and ws must
 * be re-zeroed before the next call.
 * replaces: sif_functions.compute_pc /root/reference/sif_functions.py:58-67 */
int mmb_pc_solve_mc(const double* g, int d, const double* z0, int k, int npc, int n_iter,
                    int transposed, double* pc_out, void* ws, int32_t* flag, hipStream_t stream);

/* The step's status word in one launch: out[0] = flag[0] | (nonfinite_bit if
 * any of the n values of pc is not finite), flag nullable (0).  What a
 * checked step (pipeline.FusedStep.status) reads back with one sync; the
 * eight elementwise torch kernels it replaced were ~40 us of every dataset
 * split's graph (r06 kernel trace).  A host-side helper of the drop-in's
 * error behaviour (sif_functions.py:65-67: TruncatedSVD rejects NaN).     */
int mmb_step_status(const int32_t* flag, const double* pc, int n, int32_t nonfinite_bit,
                    int32_t* out, hipStream_t stream);

/* (r06) the multi-workgroup solve runs (n_iter - 1) / 2 of its products by
 * G2 = G G (npc = 1, n_iter >= 3; the first product is by G, and extra
 * workgroups of the same launch form G2 beside it): ws holds G2 too, so
 * mmb_pc_solve_mc_ws_bytes grew by d * d * 8 bytes (an ABI change: size ws
 * with this call), and the third control word counts the squaring
 * workgroups (the first 16 bytes are still the block a caller re-zeroes
 * after MMB_FLAG_SYNC_TIMEOUT).                                             */
size_t mmb_pc_solve_mc_ws_bytes(int d);
/* The transposed branch (n < d) of mmb_pc_solve_mc from the rows themselves:
 * z0 = X^T omega [n, k] (x f32 [n, d], the a2 rows) and G2 formed in ONE
 * launch into ws (which holds both; mmb_pc_solve_mc_ws_bytes), then the
 * solve -- where mmb_xt_omega + mmb_pc_solve_mc took two launches before
 * it.  The same z0 (the same per-lane sums) and PC.
 * n < d <= 320, n <= 320, k <= min(16, d) (a wider block: MMB_EINVAL).
 * replaces: sif_functions.compute_pc for a split of n < d rows
 *   /root/reference/sif_functions.py:58-67 (sklearn extmath.py:562-566)    */
int mmb_pc_solve_mc_xt(const double* g, int d, const float* x, int64_t n, const double* omega,
                       int k, int npc, int n_iter, double* pc_out, void* ws, int32_t* flag,
                       hipStream_t stream);

/* ---------------------------------------------------------------- a4
 * out[i] = x_i - sum_c (x_i . pc_c) pc_c   in float64, x_i = num[i]/cnt[i]
 * (cnt nullable).  Exactly one of out32 / out64 non-null.
 * replaces: sif_functions.remove_pc /root/reference/sif_functions.py:69-81 */
int mmb_pc_remove(const float* num, const float* cnt, int64_t n, int d, const double* pc,
                  int npc, float* out32, double* out64, hipStream_t stream);

/* float64 X (the numpy drop-ins' general input, when it is not
 * f32-representable): the same Gram (fp64 MFMA, 64x64 blocks), start block
 * X^T Omega and f64 removal reading f64 rows, so compute_pc / remove_pc do not
 * round X to f32 first.  ws as for mmb_gram_workspace_bytes(n, d).
 * replaces: sif_functions.compute_pc / remove_pc on float64 input
 *   /root/reference/sif_functions.py:58-81                                   */
int mmb_gram_f64(const double* x, int64_t n, int d, double* g, int accumulate, void* ws,
                 hipStream_t stream);
int mmb_xt_omega_f64(const double* x, int64_t n, int d, const double* omega, int k, double* z0,
                     hipStream_t stream);
int mmb_pc_remove_f64(const double* x, int64_t n, int d, const double* pc, int npc,
                      double* out64, hipStream_t stream);

/* Streams restricted to a subset of the CUs (hipExtStreamCreateWithCUMask):
 * bit i of cu_mask[i / 32] enables CU i.  Used to run the HBM-bound stream
 * kernel and the MFMA-bound projection side by side on disjoint CUs.
 * mmb_cu_count writes the device's CU count.  No reference counterpart
 * (scheduling only).                                                         */
int mmb_cu_count(int device, int* out);

/* Bandwidth probes (measurement only, no reference counterpart): the
 * same-process HBM ceilings the bench quotes beside the 8 TB/s spec (SURVEY.md
 * §8d "a measured stream-copy ceiling").  16-byte words (nt != 0: non-temporal
 * loads / stores), four loads in flight per lane, a grid of min(blocks,
 * bytes / 4 KB) 256-thread workgroups.  mmb_probe_copy: dst = src (2 * bytes moved).  mmb_probe_read:
 * reads src once and writes one word per workgroup into sink[blocks].
 * bytes and both pointers must be 16-byte aligned.                           */
int mmb_probe_copy(const void* src, void* dst, int64_t bytes, int blocks, int nt,
                   hipStream_t stream);
int mmb_probe_read(const void* src, int64_t bytes, int blocks, int nt, uint32_t* sink,
                   hipStream_t stream);
int mmb_stream_create_cu_mask(const uint32_t* cu_mask, int mask_words, hipStream_t* out);
int mmb_stream_destroy(hipStream_t stream);

/* Host helper: numpy RandomState(seed).normal(size=count) (MT19937 +
 * legacy polar Box-Muller), written to host memory.  Used for the
 * randomized-SVD start block Omega.                                          */
int mmb_host_randn(uint32_t seed, int64_t count, double* host_out);

/* ---------------------------------------------------------------- a7
 * q_mean = (x-b)/exp(2 ls), q_sigma = (x-b)^2/exp(2 ls) - 1 over [n*t, f].
 * replaces: sif2.calc_weights /root/reference/sif2.py:103-114               */
int mmb_calc_weights(const float* x, int64_t rows, int f, const float* b_mean,
                     const float* b_log_sigma, float* q_mean, float* q_sigma, hipStream_t stream);

/* ---------------------------------------------------------------- a6+a7+a8 (stream)
 * One pass over every utterance's text tokens and audio/visual frames.
 * Text rows come from the table by id (ids non-null; wtab32 gives the weights)
 * or from dense [n,t,d] tensors (ids null: text_dense for the modality sums,
 * emb_dense for the weighted sum, w_dense [n,t] the sentence weights).
 * Writes, per utterance i:
 *   num[i,:d]  = (sum_t w_t E_t) / count_nonzero(w)  (the a2 row x_i, f32
 *                division as sif_functions.py:55; NaN when every weight is 0)
 *   s[i,:]     = [Sx_e | Sxx_e | Sx_a | Sxx_a | Sx_v | Sxx_v | 0-pad]  (sum
 *                over t of x and x^2 per feature; row stride mmb_mm2_k());
 *                s_half = 0: fp32 [n][k]; s_half = 1: fp16 [n][2][k], the hi
 *                and lo (residual) planes of s[i,:] * aux[2][i] -- the A
 *                operand of mmb_mm2_project_x3 (same bytes per row)
 *   aux[0][i]  = count_nonzero(w), aux[1][i] = sum_t w_t, aux[2][i] = the
 *                power-of-2 scale putting max|s[i,:]| in [2^14, 2^15) (planar
 *                [3][n]; aux[0] is the SIF count the Gram / removal kernels take)
 * Widths: a modality row of whole float4 units (width % 4 == 0, 16-byte
 * aligned base) may be up to 1280 floats wide, any other row up to 320;
 * MMB_EINVAL before any launch past that (and with colmax at d > 640).
 * replaces the frame loops of sif2.estimate_embedding_overall_gpu2
 *   /root/reference/sif2.py:181-205 and the gathers at simplesif.py:862-871 */
int mmb_mm2_stream(const int32_t* ids, const float* table, int64_t v, const float* wtab32,
                   const float* text_dense, const float* emb_dense, const float* w_dense,
                   const float* audio, const float* visual, int64_t n, int t, int d, int a,
                   int vd, float* num_out, void* s_out, int s_half, float* aux_out,
                   int32_t* flag, uint32_t* colmax, void* colmax_ws, hipStream_t stream);

/* mmb_mm2_stream on audio / visual frames kept in 16-bit storage.  Text is
 * gathered (ids + table, weights from wtab32 or per token from w_dense); both
 * frame tensors, [n,t,a] and [n,t,vd] contiguous, hold elements of
 * frame_type.  A frame value is widened to f32 in registers right after its
 * (non-temporal) load -- exact for both 16-bit types, fp16 subnormals
 * included -- and summed by the statements of mmb_mm2_stream in their order:
 * every output is bit for bit what mmb_mm2_stream writes for the same frames
 * upcast to f32 by the caller (where that call takes the same kernel: the
 * 16-bit types never take its narrow-frame route).  The library rounds
 * nothing: the caller chose the 16-bit values.  Outputs, layouts, the empty
 * call and the flag bits are mmb_mm2_stream's.
 * MMB_FRAMES_F32 is mmb_mm2_stream itself for the same arguments.
 * 16-bit frames: the wave kernel at t <= 64, widths % 4 == 0 and <= 512,
 * table / num_out / s_out 16-byte and audio / visual 8-byte aligned (a
 * column unit is 4 values = one 8-byte load); otherwise the workgroup kernel,
 * a modality in 4-value units when its width % 4 == 0 and its base is 8-byte
 * aligned (up to 1280 wide), in scalar 2-byte loads if not (up to 320).
 * MMB_EINVAL before any launch: a frame_type outside 0..2, a 16-bit frame
 * base that is not 2-byte aligned, anything mmb_mm2_stream rejects.
 * replaces the frame loops of sif2.estimate_embedding_overall_gpu2
 *   /root/reference/sif2.py:181-205 (which reads f32 frames only)            */
#define MMB_FRAMES_F32 0
#define MMB_FRAMES_F16 1 /* IEEE binary16 */
#define MMB_FRAMES_BF16 2
int mmb_mm2_stream_ft(const int32_t* ids, const float* table, int64_t v, const float* wtab32,
                      const float* w_dense, const void* audio, const void* visual, int frame_type,
                      int64_t n, int t, int d, int a, int vd, float* num_out, void* s_out,
                      int s_half, float* aux_out, int32_t* flag, uint32_t* colmax,
                      void* colmax_ws, hipStream_t stream);

/* mmb_mm2_stream_ft on a word table kept in 16-bit storage as well: table
 * [v,d] contiguous holds elements of table_type (MMB_TABLE_*, as
 * mmb_sif_wavg_tt), the frames elements of frame_type; all nine pairs are
 * taken.  Text is gathered (ids + table, weights from wtab32 or per token from
 * w_dense).  A table value is widened to f32 in registers right after its
 * (plain, cached) load -- exact for both 16-bit types, fp16 subnormals
 * included -- and enters the weighted sum num, the text sums Sx_e / Sxx_e,
 * the workgroup kernel's row-0 shortcut (row 0 once, as w0 E0, c0 E0,
 * c0 E0^2) and the column bounds by the statements of mmb_mm2_stream in their
 * order: x, s (both s_half formats), the three aux planes, the column bounds
 * and the flag word are bit for bit what mmb_mm2_stream_ft writes for the same
 * table upcast to f32 by the caller (where that call takes the same kernel: a
 * 16-bit table never takes the narrow-frame route, whose frame sums are in
 * another order).  The library rounds nothing.  Outputs, layouts, the empty
 * call and the flag bits are mmb_mm2_stream's.
 * MMB_TABLE_F32 is mmb_mm2_stream_ft itself for the same arguments.
 * 16-bit table: the wave kernel at t <= 64, widths % 4 == 0 and <= 512, table
 * 8-byte and num_out / s_out 16-byte aligned, the frames aligned to a unit of
 * their own type (a text column unit is 4 values = one 8-byte load);
 * otherwise the workgroup kernel, the text in 4-value units when d % 4 == 0
 * and the table is 8-byte aligned (d up to 1280), in scalar 2-byte loads if
 * not (d up to 320); the frames follow mmb_mm2_stream_ft's rules for their
 * type.
 * MMB_EINVAL before any launch: a table_type outside 0..2 (also with n == 0),
 * a 16-bit table that is not 2-byte aligned, null ids, anything
 * mmb_mm2_stream_ft rejects.
 * replaces the frame loops of sif2.estimate_embedding_overall_gpu2
 *   /root/reference/sif2.py:181-205 and the gathers at simplesif.py:862-871
 *   (which read an f32 table only)                                           */
int mmb_mm2_stream_tt(const int32_t* ids, const void* table, int table_type, int64_t v,
                      const float* wtab32, const float* w_dense, const void* audio,
                      const void* visual, int frame_type, int64_t n, int t, int d, int a, int vd,
                      float* num_out, void* s_out, int s_half, float* aux_out, int32_t* flag,
                      uint32_t* colmax, void* colmax_ws, hipStream_t stream);

/* mmb_mm2_stream for a few long rows (POM's splits: 100 / 203 transcripts of
 * 1089 / 1357 tokens), split over workgroups: every utterance is cut into P
 * token / frame ranges (parts = 0: mmb_mm2_stream_split_parts, about one
 * workgroup per CU in all; parts > 0: that many, at most t), each range
 * summed by a text, an audio and a visual workgroup of its own whose
 * partial sums go to ws (mmb_mm2_stream_split_ws_bytes(n, t, d, a, vd, parts) bytes,
 * caller-owned scratch), and a second kernel adds an utterance's partials in
 * fixed part order and writes the same outputs as mmb_mm2_stream (x, s in
 * the s_half format asked for, aux, colmax; n <= 8192 with colmax).  Rows are
 * deterministic and equal mmb_mm2_stream's to the f32 order of the token and
 * frame sums (bit for bit with one range).  Widths as mmb_mm2_stream, and
 * 3 d + 2 a + 2 vd <= 2240 (the second kernel's columns): MMB_EINVAL otherwise.
 * replaces: the frame loops of sif2.estimate_embedding_overall_gpu2
 *   /root/reference/sif2.py:181-205 at the per-split call sites
 *   /root/reference/simplesif.py:308-311 (POM's long transcripts)          */
int mmb_mm2_stream_split_parts(int64_t n, int t);
size_t mmb_mm2_stream_split_ws_bytes(int64_t n, int t, int d, int a, int vd, int parts);
int mmb_mm2_stream_split(const int32_t* ids, const float* table, int64_t v, const float* wtab32,
                         const float* text_dense, const float* emb_dense, const float* w_dense,
                         const float* audio, const float* visual, int64_t n, int t, int d, int a,
                         int vd, float* num_out, void* s_out, int s_half, float* aux_out,
                         int32_t* flag, uint32_t* colmax, void* colmax_ws, int parts, void* ws,
                         size_t ws_bytes, hipStream_t stream);

/* mmb_mm2_stream_split on audio / visual frames of storage type frame_type
 * (MMB_FRAMES_*, as mmb_mm2_stream_ft): POM's long transcripts with the frames
 * kept in 16 bits.  Text is gathered (ids + table, weights from wtab32 or per
 * token from w_dense); both frame tensors, [n,t,a] and [n,t,vd] contiguous,
 * hold elements of frame_type.  Only the frame workgroups read them: a frame
 * value is widened to f32 in registers right after its (non-temporal) load --
 * exact for both 16-bit types, fp16 subnormals included -- and summed by the
 * statements of the f32 kernel in their order; the partial sums in ws are f32,
 * so the second kernel is mmb_mm2_stream_split's.  Every output -- x, s, aux,
 * the column bounds and the flag word -- is bit for bit what
 * mmb_mm2_stream_split writes, with the same parts, for the same frames upcast
 * to f32 by the caller (and, with one range, what mmb_mm2_stream_ft's
 * workgroup kernel writes).  The library rounds nothing: the caller chose the
 * 16-bit values.  parts, ws (mmb_mm2_stream_split_ws_bytes: the same bytes for
 * every frame type), outputs, layouts, the empty call (n == 0, before the
 * workspace is looked at) and the flag bits are mmb_mm2_stream_split's.
 * MMB_FRAMES_F32 is mmb_mm2_stream_split itself for the same arguments.
 * 16-bit frames: a modality in 4-value units (one 8-byte load) when its width
 * % 4 == 0 and its base is 8-byte aligned (up to 1280 wide), in scalar 2-byte
 * loads if not (up to 320); 3 d + 2 a + 2 vd <= 2240 as for f32.
 * MMB_EINVAL before any launch: a frame_type outside 0..2, null ids, a 16-bit
 * frame base that is not 2-byte aligned, anything mmb_mm2_stream_split rejects.
 * replaces: the frame loops of sif2.estimate_embedding_overall_gpu2
 *   sif2.py:181-205 (which reads f32 frames only) at the per-split call sites
 *   simplesif.py:308-311 (POM's long transcripts)                            */
int mmb_mm2_stream_split_ft(const int32_t* ids, const float* table, int64_t v, const float* wtab32,
                            const float* w_dense, const void* audio, const void* visual, int frame_type,
                            int64_t n, int t, int d, int a, int vd, float* num_out, void* s_out,
                            int s_half, float* aux_out, int32_t* flag, uint32_t* colmax,
                            void* colmax_ws, int parts, void* ws, size_t ws_bytes, hipStream_t stream);

/* mmb_mm2_stream_split_ft on a word table kept in 16-bit storage as well: table
 * [v,d] contiguous holds elements of table_type (MMB_TABLE_*, as
 * mmb_sif_wavg_tt), the frames elements of frame_type; all nine pairs are
 * taken.  Text is gathered (ids + table, weights from wtab32 or per token from
 * w_dense).  Only the text workgroups and the second kernel read the table: a
 * table value is widened to f32 in registers right after its (plain, cached)
 * load -- exact for both 16-bit types, fp16 subnormals included -- and enters
 * the weighted sum, the text sums Sx_e / Sxx_e and the row-0 shortcut (row 0
 * once, as w0 E0, c0 E0, c0 E0^2) by the statements of the f32 kernels in
 * their order; the partial sums in ws are f32 and the frame workgroups do not
 * know the table's type.  Every output -- x, s (both s_half formats), the
 * three aux planes, the column bounds and the flag word -- is bit for bit what
 * mmb_mm2_stream_split_ft writes, with the same parts, for the same table
 * upcast to f32 by the caller (and, with one range, what mmb_mm2_stream_tt's
 * workgroup kernel writes for the 16-bit table).  The library rounds nothing.
 * parts, ws (mmb_mm2_stream_split_ws_bytes: the same bytes for every table and
 * frame type), the plan (mmb_mm2_stream_split_parts), outputs, layouts, the
 * empty call (n == 0, before the workspace is looked at) and the flag bits are
 * mmb_mm2_stream_split's; like it the call never synchronises, never allocates
 * and can be captured into a graph.
 * MMB_TABLE_F32 is mmb_mm2_stream_split_ft itself for the same arguments.
 * 16-bit table: the text in 4-value units (one 8-byte load) when d % 4 == 0
 * and the table is 8-byte aligned (d up to 1280), in scalar 2-byte loads if
 * not (d up to 320); row offsets are 64-bit (id * d); the frames follow
 * mmb_mm2_stream_split_ft's rules for their type; 3 d + 2 a + 2 vd <= 2240 as
 * for f32.
 * MMB_EINVAL before any launch: a table_type outside 0..2 (also with n == 0),
 * a 16-bit table that is not 2-byte aligned, null ids, anything
 * mmb_mm2_stream_split_ft rejects.
 * replaces: the frame loops of sif2.estimate_embedding_overall_gpu2
 *   sif2.py:181-205 and the gathers at simplesif.py:862-871 (which read an f32
 *   table only) at the per-split call sites simplesif.py:308-311 (POM's long
 *   transcripts)                                                             */
int mmb_mm2_stream_split_tt(const int32_t* ids, const void* table, int table_type, int64_t v,
                            const float* wtab32, const float* w_dense, const void* audio,
                            const void* visual, int frame_type, int64_t n, int t, int d, int a, int vd,
                            float* num_out, void* s_out, int s_half, float* aux_out, int32_t* flag,
                            uint32_t* colmax, void* colmax_ws, int parts, void* ws, size_t ws_bytes,
                            hipStream_t stream);

/* mmb_mm2_stream and mmb_mm2_project_x3 in ONE kernel (the bench step's
 * MMB2 path): the same num (x), aux[0..1] and colmax outputs as mmb_mm2_stream
 * (aux[2] is the text piece's scale) and the MMB2 rows of mmb_mm2_project_x3
 * (same fp16 x3 products; within f32 rounding of its sum order), but the
 * per-utterance sums s never reach HBM: each workgroup's streaming waves
 * stream a batch of 48 utterances modality by modality and leave each
 * (utterance, modality) piece of sums in an LDS ring, its projecting waves
 * multiply each piece of the batch with the piece-ordered fp16 hi/lo split
 * of wm (wpieces from mmb_mm2_split_pieces; c0 from mmb_mm2_prepare).  Text
 * by ids (table, wtab32 or w_dense) or dense (text_dense with w_dense, the
 * weighted sum over the same rows).  Shapes: mmb_mm2_stream_project_supported
 * (t <= 64, 256 <= d < 320, a and vd <= 320, widths % 4); 16-byte aligned
 * rows.  MMB_EINVAL otherwise.
 * replaces: the frame loops and projections of sif2.estimate_embedding_overall_gpu2
 *   /root/reference/sif2.py:181-207 and the gathers at simplesif.py:862-871 */
int mmb_mm2_stream_project_supported(int t, int d, int a, int vd);
int mmb_mm2_stream_project(const int32_t* ids, const float* table, int64_t v,
                           const float* wtab32, const float* text_dense, const float* w_dense,
                           const float* audio, const float* visual, int64_t n, int t, int d,
                           int a, int vd, const void* wpieces, const float* c0, float* num_out,
                           float* aux_out, float* mmb2_out, int32_t* flag, uint32_t* colmax,
                           void* colmax_ws, hipStream_t stream);

/* mmb_mm2_stream_project on audio / visual frames of storage type frame_type
 * (MMB_FRAMES_*, as mmb_mm2_stream_ft).  Text is gathered (ids + table,
 * weights from wtab32 or per token from w_dense); both frame tensors, [n,t,a]
 * and [n,t,vd] contiguous, hold elements of frame_type.  A 16-bit column unit
 * of 4 values is one 8-byte (non-temporal) load and stays packed until its
 * frame is summed; the widening to f32 there is exact for both 16-bit types,
 * fp16 subnormals included, and the sums are the statements of the f32 kernel
 * in their order: every output -- x, the three aux planes, the MMB2 rows, the
 * column bounds and the flag word -- is bit for bit what
 * mmb_mm2_stream_project writes for the same frames upcast to f32 by the
 * caller.  The library rounds nothing: the caller chose the 16-bit values.
 * Shapes, outputs, layouts, the empty call (n == 0) and the flag bits are
 * mmb_mm2_stream_project's; like it the call never synchronises, never
 * allocates and can be captured into a graph.
 * MMB_FRAMES_F32 is mmb_mm2_stream_project itself for the same arguments.
 * MMB_EINVAL before any launch: a frame_type outside 0..2, null ids, a 16-bit
 * frame base that is not 8-byte aligned (table / num_out / wpieces stay
 * 16-byte aligned), anything mmb_mm2_stream_project rejects.
 * replaces: the frame loops and projections of sif2.estimate_embedding_overall_gpu2
 *   /root/reference/sif2.py:164-208 (which reads f32 frames only)            */
int mmb_mm2_stream_project_ft(const int32_t* ids, const float* table, int64_t v,
                              const float* wtab32, const float* w_dense, const void* audio,
                              const void* visual, int frame_type, int64_t n, int t, int d, int a,
                              int vd, const void* wpieces, const float* c0, float* num_out,
                              float* aux_out, float* mmb2_out, int32_t* flag, uint32_t* colmax,
                              void* colmax_ws, hipStream_t stream);

/* mmb_mm2_stream_project_ft on a word table kept in 16-bit storage as well:
 * table [v,d] contiguous holds elements of table_type (MMB_TABLE_*, as
 * mmb_mm2_stream_tt), the frames elements of frame_type; all nine pairs are
 * taken.  Text is gathered (ids + table, weights from wtab32 or per token
 * from w_dense).  A 16-bit column unit of a gathered row is one 8-byte
 * (plain, cached: the rows are the reused data) load and stays packed until
 * the row is summed; the widening to f32 there is exact for both 16-bit
 * types, fp16 subnormals included, and the sums are the statements of the
 * f32-table kernel in their order: every output -- x, the three aux planes,
 * the MMB2 rows, the column bounds and the flag word -- is bit for bit what
 * mmb_mm2_stream_project_ft writes for the same table upcast to f32 by the
 * caller, for each frame type.  The library rounds nothing: the caller chose
 * the 16-bit values.  Shapes, outputs, layouts, the empty call (n == 0) and
 * the flag bits are mmb_mm2_stream_project_ft's; like it the call never
 * synchronises, never allocates and can be captured into a graph.  The
 * pipelined streamers address the table through one buffer descriptor, so a
 * table of v d sizeof(element) >= 2^31 bytes takes the group-at-a-time
 * streamer (the same rows): a 16-bit table keeps the pipelined one up to
 * twice the rows of an f32 table.
 * MMB_TABLE_F32 is mmb_mm2_stream_project_ft itself for the same arguments.
 * MMB_EINVAL before any launch: a table_type or frame_type outside 0..2 (also
 * with n == 0), null ids, a 16-bit table base that is not 8-byte aligned
 * (num_out / wpieces stay 16-byte aligned, the frames aligned to a unit of
 * their own type), anything mmb_mm2_stream_project_ft rejects.
 * replaces: the frame loops and projections of sif2.estimate_embedding_overall_gpu2
 *   /root/reference/sif2.py:164-208 and the gathers at simplesif.py:862-871
 *   (which read an f32 table and f32 frames only)                            */
int mmb_mm2_stream_project_tt(const int32_t* ids, const void* table, int table_type, int64_t v,
                              const float* wtab32, const float* w_dense, const void* audio,
                              const void* visual, int frame_type, int64_t n, int t, int d, int a,
                              int vd, const void* wpieces, const float* c0, float* num_out,
                              float* aux_out, float* mmb2_out, int32_t* flag, uint32_t* colmax,
                              void* colmax_ws, hipStream_t stream);

/* mmb_mm2_project_x3_rmpc for a few rows (the dataset splits: 100-1,284
 * rows put one or a few workgroups through the whole K loop), split over K:
 * slices (0: mmb_mm2_project_x3_split_slices) workgroups per 128-row tile
 * each run a contiguous range of the 32-deep K chunks and write their raw
 * accumulators to ws (mmb_mm2_project_x3_split_ws_bytes(n, k, slices) bytes,
 * 16-byte aligned scratch), then one launch sums each tile's slices in slice
 * order and runs the same row-wise epilogue (ldw = 320, 256 <= d < 320;
 * other shapes, or one slice, take mmb_mm2_project_x3_rmpc unchanged).  MMB2
 * and PC-removed rows equal the one-pass kernel's to the f32 order of the K
 * sum.
 * replaces: the projections of sif2.estimate_embedding_overall_gpu2
 *   /root/reference/sif2.py:187-207 at the per-split call sites
 *   /root/reference/simplesif.py:308-311                                   */
int mmb_mm2_project_x3_split_slices(int64_t n, int k);
size_t mmb_mm2_project_x3_split_ws_bytes(int64_t n, int k, int slices);
int mmb_mm2_project_x3_split(const void* s_split, const float* num, const float* aux,
                             const void* wsplit, int ldw, const float* c0, int64_t n, int k, int d,
                             float* out, const double* pc, float* sif_out, int slices, void* ws,
                             size_t ws_bytes, hipStream_t stream);

/* The fp16 hi/lo split of wm [k, ldw] (mmb_mm2_prepare) in piece order for
 * mmb_mm2_stream_project: each modality's 2 w_m rows [Sx_m | Sxx_m] padded
 * to a multiple of 32, chunks and column scales as mmb_mm2_split_bytes'
 * image, then the per-column 1/scale [ldw] f32.                             */
size_t mmb_mm2_split_pieces_bytes(int d, int a, int vd);
int mmb_mm2_split_pieces(const float* wm, int d, int a, int vd, int ldw, void* img,
                         hipStream_t stream);

/* colmax (nullable; d <= 640): the column bounds max_i |num[i,:]| of the a2
 * rows as float bits, the input of mmb_gram_i8 -- a by-product of the stream
 * kernel (per-wave running maxima into colmax_ws, then one fixed-order reduce
 * launch) instead of a second pass over x.  colmax_ws: scratch of
 * mmb_mm2_colmax_ws_bytes(d) bytes (its last 16 bytes: the batch counter of
 * mmb_mm2_stream_project's dynamic batch order, zeroed by that call itself;
 * one launch at a time per workspace).  ABI note (r05): the size grew by those
 * 16 bytes; a workspace sized by hand from the r04 formula (8192 x d floats)
 * is too small and nothing can check it -- always size it with this call.   */
size_t mmb_mm2_colmax_ws_bytes(int d);

/* Padded width (row stride) of the per-utterance sums: roundup(2(d+a+vd), 32). */
int mmb_mm2_k(int d, int a, int vd);

/* Leading dimension of the merged projection: roundup(d+1, 64).  The
 * projections take ldw <= 384 (d <= 383); mmb_mm2_prepare and mmb_mm2_project
 * return MMB_EINVAL past it, mmb_mm2_project_x3* past ldw = 320 (d <= 319). */
int mmb_mm2_ldw(int d);

/* Merge the 6 combinations' (W_mu, b_mu, W_log_sigma, b_log_sigma) into
 * wm [k, ldw] (ldw >= d+1; column d carries the total-weight row) and
 * c0 [ldw] for frame count t.  Pointer arrays are HOST arrays of DEVICE
 * pointers in key order audio, visual, audiovisual, textaudio, textvisual,
 * textaudiovisual (sif2.py:167-174).  d <= 383 (ldw <= 384: the widest wm a
 * projection takes), MMB_EINVAL before any launch otherwise.                 */
int mmb_mm2_prepare(const float* const* w_mu, const float* const* b_mu,
                    const float* const* w_ls, const float* const* b_ls, int d, int a, int vd,
                    int t, float* wm, int ldw, float* c0, void* wsplit, hipStream_t stream);

/* Bytes of the fp16 hi/lo split of wm written by mmb_mm2_prepare when wsplit
 * is non-null: per 32-deep K chunk, the hi and lo planes [ldw][32] of the
 * column-scaled wm (16-byte slots swizzled as mmb_mm2_project_x3 stages
 * them), then the per-column 1/scale [ldw] f32.                             */
size_t mmb_mm2_split_bytes(int d, int a, int vd);

/* cs = (t + s @ wm[:, :d] + c0) / (aux[1] + s @ wm[:, d] + c0[d]) with the
 * weighted text sum t = num * aux[0] (0 where aux[0] == 0), num as
 * mmb_mm2_stream writes it; out = cs / ||cs||_2 (fp32 MFMA GEMM + fused
 * epilogue).
 * replaces: sif2.py:186-207                                                  */
int mmb_mm2_project(const float* s, const float* num, const float* aux, const float* wm,
                    int ldw, const float* c0, int64_t n, int k, int d, float* out,
                    hipStream_t stream);

/* The same projection on the fp16 MFMA pipe: s (scaled per row by aux[2]) and
 * wm (scaled per column) split into fp16 hi + lo, a*b ~ ah*bh + ah*bl + al*bh
 * (3 f16 MFMAs, ~22-bit operands, fp32 accumulation).  s_split is the
 * s_half = 1 output of mmb_mm2_stream, wsplit from mmb_mm2_prepare; d < 320.
 * The bench path.                                                            */
int mmb_mm2_project_x3(const void* s_split, const float* num, const float* aux, const void* wsplit,
                       int ldw, const float* c0, int64_t n, int k, int d, float* out,
                       hipStream_t stream);

/* mmb_mm2_project_x3 with the first-PC removal of the a2 rows fused into its
 * epilogue (npc = 1): sif_out[i,:] = num[i,:] - (num[i,:] . pc) pc in f64,
 * rounded to f32 -- what mmb_pc_remove(num, NULL, n, d, pc, 1, sif_out, NULL)
 * writes, without re-reading num.  pc and sif_out both null = plain x3.
 * replaces: sif2.py:186-207 and sif_functions.remove_pc
 *   /root/reference/sif_functions.py:69-81 (npc = 1 branch :77-78)           */
int mmb_mm2_project_x3_rmpc(const void* s_split, const float* num, const float* aux,
                            const void* wsplit, int ldw, const float* c0, int64_t n, int k, int d,
                            float* out, const double* pc, float* sif_out, hipStream_t stream);

/* MMB2 at narrow frame widths (MOSI) in ONE kernel, a1-a8's stream and the
 * projection fused: the text rows of the merged projection are applied per
 * vocabulary row (text cache: P[v] = E_v Wm_t1 + E_v^2 Wm_t2, f64 rounded
 * once; the 32 words of smallest SIF weight kept in LDS), so only the
 * audio / visual frame sums (K = kq(A) + kq(Vd) <= 256) meet the f16 x3 MFMA,
 * inside the same launch; the frame sums never reach HBM.  Writes x (the a2
 * rows: mmb_mm2_stream's sums in another order -- hot words first -- so
 * equal to f32 rounding), aux, the MMB2 rows and (colmax non-null) the
 * column bounds of x for mmb_gram_i8.
 *   mmb_mm2_text_cache: cache of mmb_mm2_text_cache_bytes(v, d) bytes (16-B
 *   aligned) from the word table, the f32 weight table and the merged Wm
 *   (mmb_mm2_prepare); rebuild it when any of them changes (the launch reads
 *   the token weights from the cache's copy of wtab32).  v <= 16384.  The
 *   build writes every byte of the cache except, for a table of v < 32 words,
 *   the hot-word id slots v .. 31 (bytes [4 * 610 v, 4 * (609 v + 32)) of
 *   the cache: rows of 608 floats, v hot-slot words, then the 32 ids): the
 *   fused kernel reads min(v, 32) of them.
 *   wpieces: the piece-ordered weight split (mmb_mm2_split_pieces).
 * replaces: sif2.calc_weights + estimate_embedding_overall_gpu2
 *   /root/reference/sif2.py:103-114,164-208 with the text gather of
 *   /root/reference/simplesif.py:862-871 and sif_functions.py:28-56      */
size_t mmb_mm2_text_cache_bytes(int64_t v, int d);
int mmb_mm2_text_cache(const float* table, int64_t v, int d, const float* wtab32, const float* wm,
                       int ldw, void* cache, hipStream_t stream);
int mmb_mm2_stream_project_narrow_supported(int t, int d, int a, int vd, int64_t v);
int mmb_mm2_stream_project_narrow(const int32_t* ids, const float* table, int64_t v,
                                  const float* wtab32, const void* text_cache, const float* audio,
                                  const float* visual, int64_t n, int t, int d, int a, int vd,
                                  const void* wpieces, const float* c0, float* num_out,
                                  float* aux_out, float* mmb2_out, int32_t* flag, uint32_t* colmax,
                                  void* colmax_ws, hipStream_t stream);

/* mmb_mm2_stream_project_narrow on audio / visual frames of storage type
 * frame_type (MMB_FRAMES_*, as mmb_mm2_stream_ft); both frame tensors,
 * [n,t,a] and [n,t,vd] contiguous, hold elements of frame_type.  A frame
 * instruction keeps its lane mapping (several frame rows per load, a column
 * unit of 4 values per lane); a 16-bit unit is one 8-byte (non-temporal) load
 * and stays packed until its frame is summed.  The widening to f32 there is
 * exact for both 16-bit types, fp16 subnormals included, and the sums are the
 * statements of the f32 kernel in their order: every output -- x, the three
 * aux planes, the MMB2 rows, the column bounds and the flag word -- is bit
 * for bit what mmb_mm2_stream_project_narrow writes for the same frames
 * upcast to f32 by the caller.  The library rounds nothing: the caller chose
 * the 16-bit values.  Shapes (mmb_mm2_stream_project_narrow_supported),
 * outputs, layouts, the empty call (n == 0) and the flag bits are
 * mmb_mm2_stream_project_narrow's; like it the call never synchronises, never
 * allocates and can be captured into a graph.
 * MMB_FRAMES_F32 is mmb_mm2_stream_project_narrow itself for the same
 * arguments.
 * MMB_EINVAL before any launch, every output untouched: a frame_type outside
 * 0..2, a 16-bit frame base that is not 8-byte aligned (table, text cache,
 * num_out, mmb2_out and wpieces stay 16-byte aligned), anything
 * mmb_mm2_stream_project_narrow rejects.
 * replaces: sif2.calc_weights + estimate_embedding_overall_gpu2
 *   /root/reference/sif2.py:103-114,164-208 (which reads f32 frames only)    */
int mmb_mm2_stream_project_narrow_ft(const int32_t* ids, const float* table, int64_t v,
                                     const float* wtab32, const void* text_cache, const void* audio,
                                     const void* visual, int frame_type, int64_t n, int t, int d,
                                     int a, int vd, const void* wpieces, const float* c0,
                                     float* num_out, float* aux_out, float* mmb2_out, int32_t* flag,
                                     uint32_t* colmax, void* colmax_ws, hipStream_t stream);

/* mmb_mm2_text_cache from a word table kept in 16-bit storage: table [v,d]
 * contiguous holds elements of table_type (MMB_TABLE_*, as mmb_sif_wavg_tt).
 * A table value is widened to f32 right after its (scalar 2-byte) load --
 * exact for both 16-bit types, fp16 subnormals included: the E half of a cache
 * row is the widened value, the P half the same f64 fma chain over it, rounded
 * once.  The cache has mmb_mm2_text_cache's layout and
 * mmb_mm2_text_cache_bytes(v, d) bytes and is byte for byte the cache
 * mmb_mm2_text_cache builds from the same table upcast to f32 by the caller
 * -- the hot-word id slots v .. 31 of a table of v < 32 words stay unwritten,
 * as there.  The library rounds nothing.  Rebuild rules, v <= 16384 and the
 * 16-byte aligned cache are mmb_mm2_text_cache's; like it the call never
 * synchronises, never allocates and can be captured into a graph.  There is
 * no empty call (v > 0).
 * MMB_TABLE_F32 is mmb_mm2_text_cache itself for the same arguments.
 * MMB_EINVAL before any launch: a table_type outside 0..2, a 16-bit table that
 * is not 2-byte aligned, anything mmb_mm2_text_cache rejects.
 * replaces: the text rows of sif2.estimate_embedding_overall_gpu2
 *   /root/reference/sif2.py:186-205 over the gathers at simplesif.py:862-871
 *   (which read an f32 table only)                                           */
int mmb_mm2_text_cache_tt(const void* table, int table_type, int64_t v, int d, const float* wtab32,
                          const float* wm, int ldw, void* cache, hipStream_t stream);

/* mmb_mm2_stream_project_narrow_ft for a word table kept in 16-bit storage:
 * table [v,d] contiguous holds elements of table_type (MMB_TABLE_*), the
 * frames elements of frame_type; all nine pairs are taken.  The kernel takes
 * its text -- table rows and their projections -- from the text cache (f32
 * E | P rows, here built by mmb_mm2_text_cache_tt from the same table) and
 * the token weights from the cache's copy of wtab32: `table` is NOT read by
 * the launch, so the table's type selects no other kernel and only sets what
 * the pointer is held to.  Every output -- x, the three aux planes, the MMB2
 * rows, the column bounds and the flag word -- is bit for bit what
 * mmb_mm2_stream_project_narrow_ft writes for the same table upcast to f32 by
 * the caller with a cache built from it.  The library rounds nothing.  Shapes
 * (mmb_mm2_stream_project_narrow_supported, unchanged), outputs, layouts, the
 * empty call (n == 0) and the flag bits are mmb_mm2_stream_project_narrow's;
 * like it the call never synchronises, never allocates and can be captured
 * into a graph.
 * MMB_TABLE_F32 is mmb_mm2_stream_project_narrow_ft itself for the same
 * arguments (a 16-byte aligned table).
 * MMB_EINVAL before any launch, every output untouched: a table_type outside
 * 0..2 (also with n == 0), a 16-bit table that is not 2-byte aligned (its
 * element; text cache, num_out, mmb2_out and wpieces stay 16-byte aligned,
 * the frames aligned to a unit of their type), anything
 * mmb_mm2_stream_project_narrow_ft rejects.
 * replaces: sif2.calc_weights + estimate_embedding_overall_gpu2
 *   /root/reference/sif2.py:103-114,164-208 with the text gather of
 *   /root/reference/simplesif.py:862-871 (which reads an f32 table only)     */
int mmb_mm2_stream_project_narrow_tt(const int32_t* ids, const void* table, int table_type, int64_t v,
                                     const float* wtab32, const void* text_cache, const void* audio,
                                     const void* visual, int frame_type, int64_t n, int t, int d,
                                     int a, int vd, const void* wpieces, const float* c0,
                                     float* num_out, float* aux_out, float* mmb2_out, int32_t* flag,
                                     uint32_t* colmax, void* colmax_ws, hipStream_t stream);

/* ---------------------------------------------------------------- a10/a11
 * SentimentModel(d -> h -> o): y = squeeze(W2 relu(W1 x + b1) + b2).
 * Forward for rows idx[0..b) (idx nullable = 0..b) of latents [*, d].
 * replaces: sentiment_model.SentimentModel.forward /root/reference/sentiment_model.py:36-41 */
int mmb_mlp_forward(const float* latents, const int64_t* idx, int64_t b, int d, int h, int o,
                    const float* w1, const float* b1, const float* w2, const float* b2,
                    float* y_out, hipStream_t stream);

/* Differentiable forward / backward of the same model, for the e2e joint
 * objective whose regressor term backpropagates into the latents
 * (simplesif.py:776-790, autograd of sentiment_model.py:36-41):
 *   forward_train: y [b,o] and the post-ReLU hidden activations hid [b,h];
 *   backward: dh_ws [b,h] scratch, dx [b,d] (nullable), dw1 [h,d], db1 [h],
 *   dw2 [o,h], db2 [o] (each nullable) for upstream gradient dy [b,o].
 * Parameter gradients reduce over the rows in a fixed order.                 */
int mmb_mlp_forward_train(const float* x, int64_t b, int d, int h, int o, const float* w1,
                          const float* b1, const float* w2, const float* b2, float* y_out,
                          float* hid_out, hipStream_t stream);
int mmb_mlp_backward(const float* x, const float* hid, int64_t b, int d, int h, int o,
                     const float* w1, const float* w2, const float* dy, float* dh_ws, float* dx,
                     float* dw1, float* db1, float* dw2, float* db2, hipStream_t stream);

/* L1 loss sum for prediction rows vs labels (per-batch means written to
 * batch_loss): the evaluation loops of sentiment_model.py:60-74,117-125.
 * Batches are consecutive slices of `perm` of size batch (last one ragged). */
int mmb_mlp_eval(const float* latents, const float* labels, const int64_t* perm, int64_t n,
                 int batch, int d, int h, int o, const float* w1, const float* b1,
                 const float* w2, const float* b2, float* batch_loss, float* pred_out,
                 hipStream_t stream);

/* SGD training of the regressor over n_epochs epochs of mini-batches drawn
 * from `perm` (the DataLoader order: epochs concatenated, batches of `batch`
 * rows, the last one ragged), with loss = L1(reduction='none').mean() and
 * p -= lr * grad, all in ONE launch of ceil(h / 32) workgroups (one 32-wide
 * hidden tile each, exchanging their output shares once per mini-batch).
 * Parameters are updated in place; per-step losses go to step_loss
 * [n_epochs * ceil(n_per_epoch / batch)].  With v_latents non-null the
 * launch also runs the validation passes: after every epoch e with
 * (epoch0 + e) % valid_every == 0 the per-batch mean L1 of the validation rows
 * v_perm[k * n_valid ...] (k = the k-th such epoch of this launch) with the
 * weights of that moment go to valid_loss[k * ceil(n_valid / batch) + j].
 * ws: scratch of mmb_mlp_workspace_bytes(d, h) bytes (16-B aligned), ZEROED
 * by the caller before its first use (a completed launch leaves ALL of it
 * zero, the exchange slots it used as well as the control words);
 * flag (nullable) gets MMB_FLAG_SYNC_TIMEOUT if the workgroups' exchange
 * stalls (~1 s) or finds ws dirty (the parameters are then invalid and ws
 * must be re-zeroed).  The P = ceil(h / 32) workgroups are launched
 * cooperatively (co-resident, or the launch fails) after an occupancy check
 * (MMB_EINVAL when the device cannot hold them at once).  h <= 512,
 * n_out <= 16, batch <= 32, d % 4 == 0 and d <= mmb_mlp_train_max_d(n_out):
 * 448 for n_out <= 13, 416 for n_out = 14..16 (two mini-batches of rows,
 * padded to 32 features, share the workgroup's LDS with 129 n_out floats of
 * outputs; 0 for an n_out outside 1..16).  Anything else: MMB_EINVAL.
 * replaces: sentiment_model.train_sentiment loop incl. its validation passes
 *   /root/reference/sentiment_model.py:76-127                               */
size_t mmb_mlp_workspace_bytes(int d, int h);
int mmb_mlp_train_max_d(int n_out);
int mmb_mlp_train(const float* latents, const float* labels, const int64_t* perm,
                  int64_t n_per_epoch, int n_epochs, int batch, int d, int h, int o, float lr,
                  float* w1, float* b1, float* w2, float* b2, float* step_loss,
                  const float* v_latents, const float* v_labels, const int64_t* v_perm,
                  int64_t n_valid, int valid_every, int epoch0, float* valid_loss, void* ws,
                  int32_t* flag, hipStream_t stream);

/* ---------------------------------------------------------------- §8f row 1
 * Latent-optimisation likelihoods (the objective simplesif.py:49-162,708-806
 * minimises).  Word term = get_word_log_prob_angular2, losses.py:68-95;
 * Gaussian term = get_normal_log_prob, losses.py:13-33, summed per modality
 * combination by get_log_prob_matrix, losses.py:216-274.
 *
 * mmb_word_normalize: wn [v, mmb_word_pad(d)] = table / max(|row|, 1e-8),
 * zero padded (torch cosine_similarity's x2 / |x2|; done once per table).   */
int mmb_word_pad(int d);
int mmb_word_normalize(const float* table, int64_t v, int d, float* wn, hipStream_t stream);

/* lp[b] = sum_t mask[b,t] log(alpha_b w[b,t] + (1-alpha_b) score_bt / Z_b),
 * Z_b = sum_{v<V} (1 - acos(cos(l_b, table_v))/pi), alpha_b = 1/(a Z_b + 1),
 * score_bt = 1 - acos(cos(l_b, e_bt))/pi, e_bt = table[ids[b,t]] (ids non-null)
 * or sent_dense[b,t,:].  d <= 320 (forward and backward; wider: MMB_EINVAL,
 * nothing launched).  ws: scratch of
 * mmb_word_workspace_bytes(b, d, v).  With want_grad, state [b,4], gsum
 * [b, pad(d)] and cos_out [b, l] are written for mmb_word_logprob_backward.
 * replaces: losses.get_word_log_prob_angular2 /root/reference/losses.py:68-95
 *           (and get_word_log_prob_angular :36-66 with w = weights[data])  */
size_t mmb_word_workspace_bytes(int64_t b, int d, int64_t v);
int mmb_word_logprob_forward(const float* latents, int64_t b, int d, const float* wn, int64_t v,
                             const int32_t* ids, const float* table, const float* sent_dense,
                             int l, const float* w, const float* mask, float a, int want_grad,
                             void* ws, float* lp, float* state, float* gsum, float* cos_out,
                             hipStream_t stream);
/* dlat[b,:] = dlp[b] * d lp_b / d latents[b,:] (autograd of losses.py:68-95). */
int mmb_word_logprob_backward(const float* latents, int64_t b, int d, int64_t v,
                              const int32_t* ids, const float* table, const float* sent_dense,
                              int l, const float* w, const float* mask, float a,
                              const float* state, const float* gsum, const float* cosv,
                              const float* dlp, float* dlat, hipStream_t stream);

/* stats [n][3][f] f64 = per-utterance masked frame sums (sum_t m, sum_t m x,
 * sum_t m x^2) of x [n,t,f] (mask nullable = ones); streamed once per split.
 * n = 0 writes nothing (x and stats may be null); t = 0 writes zeros (x may be
 * null). */
int mmb_gauss_stats(const float* x, const float* mask, int64_t n, int t, int f, double* stats,
                    hipStream_t stream);
/* lp[k][b] = get_normal_log_prob(mu_k[b], sigma_k[b], x, mask) for combination
 * k of modalities mods[k] (bit 0 text, 1 audio, 2 visual; features in that
 * torch.cat order), from the stats of rows idx[b] (idx nullable = b).
 * stats[3] / fm[3] / mods / mu / sigma are HOST arrays (of device pointers).
 * Only sigma^2 and |sigma| enter (the reference's log(1 / sqrt(2 pi sigma^2))):
 * sigma's sign does not matter to lp, and the gradients below are those of
 * that lp for either sign (sigma != 0).  b = 0 returns MMB_OK with nothing
 * launched (the device pointers may then be null).
 * replaces: losses.get_normal_log_prob /root/reference/losses.py:13-33 and the
 *           per-modality loop of get_log_prob_matrix :249-256               */
int mmb_gauss_loglik(const double* const* stats, const int* fm, const int64_t* idx, int64_t b,
                     int nkeys, const int* mods, const float* const* mu,
                     const float* const* sigma, float* lp, hipStream_t stream);
/* dmu_k = dlp_k (M1 - mu M0)/s^2,  dsigma_k = dlp_k (Q/s^3 - M0/s)  (dmu/dsigma
 * entries nullable). */
int mmb_gauss_backward(const double* const* stats, const int* fm, const int64_t* idx, int64_t b,
                       int nkeys, const int* mods, const float* const* mu,
                       const float* const* sigma, const float* dlp, float* const* dmu,
                       float* const* dsigma, hipStream_t stream);
/* The same two with row strides (elements; HOST arrays, one per key): mu_k /
 * dmu_k rows ld_mu[k] apart, sigma_k / dsigma_k rows ld_sigma[k] apart -- the
 * per-key column blocks of the generator's fused output [B, 2 F] (mu) and of
 * exp() of its log-sigma half [B, F] (sigma) without copies.  ld >= F_k;
 * null arrays mean F_k (contiguous rows), as in the unstrided entry points. */
int mmb_gauss_loglik_strided(const double* const* stats, const int* fm, const int64_t* idx,
                             int64_t b, int nkeys, const int* mods, const float* const* mu,
                             const int64_t* ld_mu, const float* const* sigma,
                             const int64_t* ld_sigma, float* lp, hipStream_t stream);
int mmb_gauss_backward_strided(const double* const* stats, const int* fm, const int64_t* idx,
                               int64_t b, int nkeys, const int* mods, const float* const* mu,
                               const int64_t* ld_mu, const float* const* sigma,
                               const int64_t* ld_sigma, const float* dlp, float* const* dmu,
                               float* const* dsigma, hipStream_t stream);

/* Backward of the generator's LayerNorm (reference models.py:163-164,
 * nn.LayerNorm(embedding_dim); its backward is torch's).  dy, x, dx: [n, d]
 * row-major f32; mean, rstd: [n], the forward's saved statistics
 * (torch.native_layer_norm); gamma: [d].  Writes dx and, when non-null,
 * dgamma = sum_rows dy xhat and dbeta = sum_rows dy (fixed reduction order:
 * deterministic).  One launch. */
int mmb_layer_norm_backward(const float* dy, const float* x, const float* mean, const float* rstd,
                            const float* gamma, int64_t n, int d, float* dx, float* dgamma,
                            float* dbeta, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MMB_H_ */
