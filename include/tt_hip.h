/* tt_hip.h — C ABI of libtt_hip.so, the MI355X (gfx950) implementation of the
 * two-tower contrastive training step of mateomarin/two_towers.
 *
 * The reference has no native code and no FFI: its hot path is PyTorch module calls
 * (nn.GRU, nn.Linear, nn.LayerNorm, F.normalize, matmul, cross_entropy,
 * cosine_similarity, topk, optim.Adam). Each entry point below replaces one of those
 * call sites; the reference file:line it stands in for is given per function.
 * two_towers_amd/ (Python, ctypes) binds these entry points behind the reference's
 * own nn.Module surface (EnhancedTwoTowerModel, InfoNCELoss, MarginRankingLoss,
 * get_hard_negatives).
 *
 * Conventions
 *  - All pointers are device pointers (HBM) owned by the caller; nothing here
 *    allocates device memory. Scratch ("ws") is caller-provided.
 *  - dtype selects storage/arithmetic of the tensor operands: TT_DT_F32 (exact fp32
 *    MFMA) or TT_DT_BF16 (bf16 storage, fp32 accumulation). Tensors typed `float*`
 *    are always fp32.
 *  - Matrices are row-major with an explicit leading dimension in ELEMENTS.
 *  - stream is a hipStream_t (NULL = default stream); every call is stream-ordered
 *    and asynchronous. Thread-safe on distinct streams.
 *  - Return 0 on success, TT_EINVAL on a bad argument, else a hipError_t code;
 *    tt_last_error() returns a thread-local message for the last failure.
 */
#ifndef TT_HIP_H
#define TT_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TT_OK 0
#define TT_EINVAL 1000
#define TT_DT_F32 0
#define TT_DT_BF16 1

/* Library version string, e.g. "tt_hip 0.2.0 gfx950". */
const char* tt_version(void);
/* Message describing the last non-zero return on this thread ("" if none). */
const char* tt_last_error(void);
/* Kernel-variant switches (process-wide; initialised once from the environment variable
 * of the same name in upper case with a TT_ prefix, e.g. gru_step <- TT_GRU_STEP):
 * GRU: gru_step, gru_depth, gru_bwd_rows, gru_bwd_big, gru_bwd_streams, gru_bwd_persist,
 * gru_bwd_skew, gru_fwd_step_rows, gru_fwd_xc, gru_fwd_xs, gru_fwd_skew, gru_xc_coop,
 * gru_step_ring, gru_yprev (read by the callers of tt_gru_fwd_yprev, not by the kernels:
 * whether the training step uses the previous-state layout where it is supported); GEMM: gemm_persist, gemm_persist_maxk, gemm_a3, gemm_buf, gemm_bres,
 * bres_rows, bres_form, wgrad_tall, gemm_iepi, gemm_order, gemm_skew, gemm_regstage, gemm_stream_out; losses:
 * hn_gemm, hn_map, hn_scan_gemm, infonce_flash; search: rank_gemm, search_i8_qb; diagnostics gru_xc_skip, gru_xc_spins. The authoritative list with
 * defaults is kOpts in two_towers_amd/csrc/tt_gemm.hip. Every variant computes the same
 * function; they exist for A/B measurement and for tests that compare variants.
 * Not synchronised with launches in flight: set them between steps. */
int tt_set_option(const char* name, int value);
int tt_get_option(const char* name, int* value);

/* ---------------------------------------------------------------- featurisation */
/* Word2Vec row gather: out[i, :] = table[ids[i], :] for ids[i] >= 0, zero row for
 * ids[i] < 0 (pad / all-OOV).  Replaces the per-word lookup + zero padding of
 * EnhancedDataset.text_to_embedding (enhanced_two_tower.py:144-166).
 * table [vocab, ep], out [n, ep]; ep * sizeof(dtype) must be a multiple of 16. */
int tt_embed_gather(int dtype, const void* table, long vocab, int ep, const int32_t* ids, long n,
                    void* out, void* stream);

/* Packs float rows [n, e] into dtype rows [n, ep] (zero columns e..ep-1): the
 * reference's float [B,T,E] encoder input (enhanced_two_tower.py:50,56) into the
 * padded layout the projections read. */
int tt_pack_rows(int dtype, const float* src, long n, int e, int ep, void* out, void* stream);
/* Weight packing in one launch: up to 16 jobs, each dst[r][c] = src[r][c] (+ src2[r][c]) for
 * c < cols and 0 for cols <= c < dcols, r < rows, written as bf16 (dst_bf16) or fp32. cols,
 * dcols, lds, ldd multiples of 4 and src / src2 / dst 16-byte aligned. Replaces the per-step
 * torch.cat / pad / cast of the GRU weights and the folded r|z biases (towers.py _Packed). */
typedef struct {
  const float* src;
  const float* src2; /* NULL or a second fp32 operand of the same layout, added */
  void* dst;
  int rows, cols, dcols;
  long lds, ldd;
  int dst_bf16;
} tt_pack_job;
int tt_pack_multi(const tt_pack_job* jobs, int njobs, void* stream);

/* y[i] = (dtype)x[i] (fp32 -> dtype) for n elements. */
int tt_cast(int dtype, const float* x, long n, void* y, void* stream);

/* out[c] (+)= sum_r x[r*ld + c] over r < rows (x fp32). Bias gradients: summed in a
 * fixed order (no atomics), so results are bit-for-bit reproducible. */
int tt_colsum(const float* x, long rows, int cols, long ld, float* out, int accumulate, void* stream);

/* ------------------------------------------------------------------------ GEMM */
/* Batched MFMA GEMM (up to 4 independent problems of one shape per launch):
 *     C_b[m][n] = alpha * sum_k A_b(m,k) B_b(n,k) (+ bias_b[n]) (relu) (*dropmask) (+ C_b)
 * a_kouter = 0: A stored [m][k] (lda);   1: A stored [k][m] (lda).
 * b_kouter = 0: B stored [n][k] (ldb);   1: B stored [k][n] (ldb).
 * With b_kouter = 1 and bshift[b] != 0, B row k is read from row k + shift when
 * (k mod seq_t) + shift lies in [0, seq_t), else treated as zero (GRU h_{t-1} operand);
 * any shift, and k must be a multiple of seq_t (else TT_EINVAL).
 * drop_p > 0 multiplies element (m, n) by the counter-based dropout mask
 * keep(drop_seed, m, n) / (1 - drop_p) (see tt_gru_fwd).
 * splits > 1 splits K across workgroups: fp32 partials go to splitk_ws
 * (tt_gemm_ws_size floats) and are reduced into C; relu/dropout unsupported then.
 * out_dtype is TT_DT_F32 or dtype. Any m, n, k; operand base pointers and leading
 * dimensions must be 16-byte aligned (lda * sizeof(dtype) % 16 == 0).
 * Every problem runs on the hand-written MFMA kernels of this library (tt_gemm.hip,
 * tt_gemm_core.h); no vendor GEMM is linked. */
typedef struct {
  const void* a[4];
  const void* b[4];
  void* c[4];
  const float* bias[4];
  int bshift[4];
  /* a_kouter = 1 only: columns m >= a_split of A come from a_hi[b] + (m - a_split)
   * (same lda); a_split = 0 disables. Lets dW_hh read the GRU dL/dgh operand, whose
   * r|z columns live in the dL/dgx buffer, without a copy. */
  const void* a_hi[4];
  int a_split;
  /* dropout (drop_p > 0): the mask of element (m, n) is keep(drop_seed, drop_row0 + m, n) */
  uint32_t drop_row0;
} tt_gemm_batch;

int tt_gemm(int dtype, int out_dtype, int a_kouter, int b_kouter, int m, int n, int k,
            const tt_gemm_batch* batch, int nbatch, long lda, long ldb, long ldc, float alpha,
            int beta_accum, int relu, int seq_t, uint32_t drop_seed, float drop_p, int splits,
            float* splitk_ws, void* stream);
/* tt_gemm with C stored transposed when c_trans != 0: C_b[n][m] with ldc >= m (bias still
 * per n). The split-K reduction writes it, summing the slices in the same order, so the
 * values are those of tt_gemm: it needs splits > 1 after tt_gemm's clamping to the K-tiles
 * (an error otherwise). The layer-0 dW_ih, computed as X0^T dG, lands as [3H, Ep]. */
int tt_gemm_ct(int dtype, int out_dtype, int a_kouter, int b_kouter, int m, int n, int k,
               const tt_gemm_batch* batch, int nbatch, long lda, long ldb, long ldc, float alpha,
               int beta_accum, int relu, int seq_t, uint32_t drop_seed, float drop_p, int splits,
               float* splitk_ws, int c_trans, void* stream);
/* fp32 elements of splitk_ws: the split partials for splits > 1, else 0. */
long tt_gemm_ws_size(int m, int n, int nbatch, int splits);
/* Heuristic split count for a (m, n, k, nbatch) problem. */
int tt_gemm_pick_splits(int m, int n, int k, int nbatch);
/* What the last tt_gemm / tt_gemm_ct call on this thread launched: one TT_GK_* family code
 * (value & TT_GK_MASK) plus TT_GKF_* flag bits. TT_GK_NONE after a call that failed its
 * argument checks or had nothing to do (m or n zero). For tests, which assert the kernel a
 * case was written to reach, so that a moved dispatch threshold fails loudly instead of
 * leaving a kernel untested. */
#define TT_GK_NONE 0
#define TT_GK_REG128 1  /* register-staged 128x128 (a 16-byte chunk may straddle an operand edge) */
#define TT_GK_DMA128 2  /* LDS-DMA 128x128 */
#define TT_GK_BIG8 3    /* 256x256 8-phase, one tile per workgroup */
#define TT_GK_PERSIST 4 /* 256x256 persistent */
#define TT_GK_BRES 5
#define TT_GK_WREG 6
#define TT_GK_TALL 7
#define TT_GK_W4 8
#define TT_GK_MASK 0xf
#define TT_GKF_A3 0x10          /* 8-phase / persistent: three A slots */
#define TT_GKF_BUF 0x20         /* ... operand DMAs through buffer resources */
#define TT_GKF_IEPI 0x40        /* persistent: interleaved epilogue */
#define TT_GKF_WALK 0x80        /* persistent: column-group walk (option gemm_order) */
#define TT_GKF_TALL_WHOLE 0x100 /* gemm_tall: whole 320-row tiles launched */
#define TT_GKF_TALL_HALF 0x200  /* gemm_tall: half tiles launched */
#define TT_GKF_SPLITK 0x400     /* the split-K reduction ran */
#define TT_GKF_RED4 0x800       /* ... in its 4-wide form */
int tt_gemm_last_kernel(void);
/* Which B-resident short-K kernel tt_gemm runs a bf16, a_kouter = b_kouter = 0, bias-only,
 * one-split product of this shape on (16-byte aligned C rows and biases), under the
 * current options: 0 none (the general kernels), 1 gemm_bres (a panel of B in LDS),
 * 2 gemm_wreg (B in registers, A rows through an LDS ring; option bres_form 1). */
int tt_gemm_bres_form(int m, int n, int k, int nbatch, long lda, long ldc);
/* Whether tt_gemm runs a product of this shape, under the current options, on gemm_tall
 * (option wgrad_tall: one 320-row tile per 256-column panel; bf16 K-outer operands, fp32
 * out, 256 < m <= 320): 1, else 0 (the general kernels). splits as passed to tt_gemm;
 * extras: bit 0 bias, 1 relu, 2 dropout, 3 bshift, 4 a_split, 5 beta_accum. */
int tt_gemm_tall_form(int dtype, int out_dtype, int a_kouter, int b_kouter, int m, int n, int k, long lda,
                      long ldb, int splits, int extras);

/* ------------------------------------------------------------------------- GRU */
/* One bidirectional GRU layer, forward, all time steps (torch nn.GRU semantics:
 * r = s(Wir x + bir + Whr h + bhr), z = s(Wiz x + biz + Whz h + bhz),
 * n = tanh(Win x + bin + r*(Whn h + bhn)), h' = (1-z) n + z h, h0 = 0).
 * Replaces nn.GRU at enhanced_two_tower.py:51,57 (per layer, up to 4 recurrences =
 * {query,doc} x {fwd,rev} per launch). The input projection g = x Wih^T + bih
 * (+ [bhr, bhz, 0]) is a tt_gemm done by the caller. H must be a multiple of 8 (the
 * epilogues update 8 consecutive hidden units per thread; tt_gru_bwd likewise). */
typedef struct {
  const void* g;       /* [B*T, ldg]: gate pre-activations r|z|n (3H columns)        */
  const void* whh;     /* [3H, H]                                                    */
  const float* bhn;    /* [H]                                                        */
  void* y;             /* h_t: element (b,t,j) at y[(b*T+t)*ldy + j]                 */
  void* x1;            /* optional dropout(y) for the next layer (same layout) or NULL */
  void* save;          /* [B*T, 4H] saved pre-activations of r|z|n and gh_n (backward) */
  float* hstate;       /* fp32 scratch [2][B][H] (per-step kernel only)              */
  int dir;             /* 0: t = 0..T-1 ; 1: t = T-1..0                              */
  uint32_t drop_seed;  /* dropout stream of x1                                       */
  int drop_col0;       /* column of this recurrence inside the layer output (dir*H)  */
  uint32_t drop_row0;  /* mask row of local row 0: the mask of element (b, t, col) is
                          keep(drop_seed, drop_row0 + b*T + t, drop_col0 + col), so a
                          data-parallel rank passes rank * B * T and draws the masks the
                          single-process run of the global batch would               */
} tt_gru_fwd_rec;

int tt_gru_fwd(int dtype, const tt_gru_fwd_rec* recs, int nrec, int B, int T, int H, long ldg,
               long ldy, float drop_p, void* ws, long ws_bytes, void* stream);
/* Kernel launches tt_gru_fwd issues without a workspace: 1 for the persistent bf16 kernel
 * (H % 64 == 0, H <= 512; 64 batch rows per workgroup kept resident for all T steps, hstate
 * unused), T for the per-step kernel (fp32, other H, or option gru_step = 1). */
int tt_gru_fwd_launches(int dtype, int T, int H);
/* Device scratch (bytes, 0 = none used) that lets tt_gru_fwd run the column-split persistent
 * kernel for this call shape on the current device: bf16, H 256 / 512, a batch large enough
 * (or option gru_fwd_xc = 2), and every member workgroup co-resident (one per CU, checked
 * against the occupancy query; a plain launch by default, hipLaunchCooperativeKernel with
 * option gru_xc_coop = 1). The occupancy check covers an idle device only: kernels of other
 * streams may keep members from being co-resident, and then the bounded member waits give up
 * and set the STATUS word below (outputs invalid, reported -- never silently wrong); callers
 * that overlap other work with this launch should expect that. H/64 workgroups share a block of
 * batch rows, each keeps 64 units' W_hh rows in registers, and they exchange h every step
 * through ws: per-group arrival counters (zeroed by every call, stream-ordered) and exchange
 * images. ws: 256-byte aligned, one buffer per launch in flight (distinct streams need
 * distinct buffers). NULL, or ws_bytes below the size: the row-owning kernel runs instead.
 * The first 4 bytes of ws are a STATUS word: nonzero once a launch gave up waiting for a
 * member (that launch's outputs are invalid). The library sets it and never clears it; the
 * caller zeroes it when it allocates ws and reads it back (asynchronously) after the call. */
long tt_gru_fwd_ws_size(int dtype, int nrec, int B, int T, int H, long ldg, long ldy);
/* Launches tt_gru_fwd issues for this exact call shape given a tt_gru_fwd_ws_size workspace
 * (1 where a column-split or row-owning persistent kernel applies, T for the per-step
 * kernel); needs the device. */
int tt_gru_fwd_launches_for(int dtype, int nrec, int B, int T, int H, long ldg, long ldy);

/* Inference forward of the same layer (no gradient will be taken): the recurrence of
 * tt_gru_fwd with drop_p = 0, without the saved pre-activations and the dropout copy, and
 * with the layer output optional. Every value it writes is bit-identical to what tt_gru_fwd
 * (drop_p = 0) writes at the same position: same kernels' product order and gate cell.
 *   y      given: the layer output, as tt_gru_fwd's y.
 *   hfinal given: h after the recurrence's last step (t = T-1 for dir 0, t = 0 for dir 1) of
 *          batch row b at hfinal[b*ldf + j], j < H, in dtype. The two directions of a tower
 *          may point at columns 0 and H of one [B, 2H] buffer (ldf = 2H).
 * Both may be given; at least one must be, and all records of a call must agree on which are
 * NULL (else TT_EINVAL). Alignment as tt_gru_fwd, plus (ldf * element size) % 16 == 0.
 * ws / ws_bytes follow tt_gru_fwd's contract (column-split kernel, status word at ws[0..3]);
 * tt_gru_fwd_ws_size and tt_gru_fwd_launches_for answer for this call as well (same launch
 * geometry). scratch: tt_gru_infer_scratch_size bytes per recurrence, 16-byte aligned; only
 * the per-step kernel uses it (the fp32 state, and without y the image of h_{s-1} its
 * product reads), so it is 0 / may be NULL wherever a persistent kernel applies. */
typedef struct {
  const void* g; const void* whh; const float* bhn; /* as tt_gru_fwd_rec                  */
  void* y;        /* [B*T, ldy] layer output, or NULL (final-only)                         */
  void* hfinal;   /* [B, ldf] dtype: h after the last step, or NULL                        */
  void* scratch;  /* tt_gru_infer_scratch_size bytes per recurrence (may be 0)             */
  int dir;
} tt_gru_infer_rec;
int  tt_gru_fwd_infer(int dtype, const tt_gru_infer_rec* recs, int nrec, int B, int T, int H, long ldg,
                      long ldy, long ldf, void* ws, long ws_bytes, void* stream);
/* Bytes of tt_gru_infer_rec.scratch for one recurrence of this call shape under the current
 * options (final_only: y is NULL); 0 where the state stays on chip. */
long tt_gru_infer_scratch_size(int dtype, int B, int T, int H, int final_only);

/* Backward (BPTT) of tt_gru_fwd. Produces dL/dg (= dgx, feeds dWih, dbih and the
 * layer-input gradient) and dL/dgh (feeds dWhh), plus bias partial sums: tt_gru_bias_rows(B)
 * = ceil(B / 64) rows, one per 64-row batch tile (the smallest backward tile; a kernel on
 * larger tiles fills one row per tile and leaves the rest zero), columns r|z|n|ghn; reduce
 * with tt_colsum: dbih = [0:3H], dbhh = [0:2H] ++ [3H:4H].
 * dy and dfinal are independent: either or both may be given in every kernel family; dfinal
 * enters dL/dh at the recurrence's last processed step, dy at every step. */
typedef struct {
  const void* save;    /* [B*T, 4H] from tt_gru_fwd          */
  const void* y;       /* layer output (source of h_{s-1})   */
  const void* dy;      /* dL/dy (ldy) or NULL                */
  const float* dfinal; /* dL/dh_final [B, ldf] or NULL       */
  const void* whh;     /* [3H, H]                            */
  void* dgx;           /* [B*T, ldd]: dL/d(r|z|n pre-activation), 3H columns        */
  void* dgh;           /* [B*T, ldd]: dL/d(W_hn h + b_hn), H columns; dL/dgh (the
                          dW_hh operand) is [r|z columns of dgx, this block]        */
  void* dhstate;       /* scratch [2][B][H] of dtype (carry dh*z) */
  float* dbias_part;   /* fp32 [tt_gru_bias_rows(B)][4H]; zeroed by tt_gru_bwd */
  int dir;
} tt_gru_bwd_rec;

int tt_gru_bwd(int dtype, const tt_gru_bwd_rec* recs, int nrec, int B, int T, int H, long ldy,
               long ldd, long ldf, void* stream);
/* Kernel launches tt_gru_bwd issues: 1 for the row-owning bf16 kernel (H 256 or 512: one
 * workgroup per 128 batch rows x all H units walks every step), T otherwise. */
int tt_gru_bwd_launches(int dtype, int T, int H);
/* 1 when tt_gru_bwd keeps the BPTT carry on chip (the row-owning kernel at H <= 512: no
 * carry bytes in HBM), 0 when it round-trips a bf16 / fp32 carry buffer (dhstate). */
int tt_gru_bwd_carry_on_chip(int dtype, int T, int H);
int tt_gru_bias_rows(int B);

/* Previous-state layout of the layer output. Apart from the final state, every reader of a
 * training layer's output wants the state a step STARTS from: the BPTT epilogue (h_{s-1}) and
 * dW_hh = sum_t dL/dgh[t]^T h[t-1]. tt_gru_fwd_yprev is tt_gru_fwd with y stored that way:
 *   dir 0: y[b, t] = h[b, t-1], zeros at t = 0;   dir 1: y[b, t] = h[b, t+1], zeros at t = T-1
 * (the zero rows are written by the call), and the state after the last step goes to
 * hfinal[i][b*ldf + j] (dtype; one pointer per record, or hfinal NULL: not wanted), as
 * tt_gru_fwd_infer's hfinal. save, x1 (at its own time index), the dropout draw and every
 * value computed are tt_gru_fwd's: h_t is bit for bit what tt_gru_fwd stores at row t. With
 * it dW_hh is a plain TN tt_gemm on y (no bshift / seq_t) with the same sums in the same
 * order, and tt_gru_bwd_yprev is tt_gru_bwd reading h_{s-1} at row t of that y.
 * Implemented by the column-split forward kernels (gru_fwd_xs, gru_fwd_xcp: bf16, H 256 /
 * 512, a tt_gru_fwd_ws_size workspace) and the row-owning backward (gru_bwd_rows);
 * tt_gru_yprev_supported says whether both apply to a call shape on the current device under
 * the current options. Where they do not, the two entry points return TT_EINVAL (they never
 * fall back to another layout) and the caller uses tt_gru_fwd / tt_gru_bwd. */
int tt_gru_yprev_supported(int dtype, int nrec, int B, int T, int H, long ldg, long ldy);
int tt_gru_fwd_yprev(int dtype, const tt_gru_fwd_rec* recs, void* const* hfinal, int nrec, int B, int T, int H,
                     long ldg, long ldy, long ldf, float drop_p, void* ws, long ws_bytes, void* stream);
int tt_gru_bwd_yprev(int dtype, const tt_gru_bwd_rec* recs, int nrec, int B, int T, int H, long ldy,
                     long ldd, long ldf, void* stream);

/* ------------------------------------------------------------ projection head */
/* Linear(4h->2h) -> LayerNorm(2h, eps) -> ReLU -> Linear(2h->h), fwd and bwd.
 * Replaces query_proj/doc_proj (enhanced_two_tower.py:36-48, applied :54,60).
 * Weights in dtype (w1 [2h,4h], w2 [h,2h]); biases/LN affine fp32. */
typedef struct {
  const void* w1; const float* b1; const float* ln_g; const float* ln_b;
  const void* w2; const float* b2;
  const void* x;   /* [B, 4h] dtype : cat(h_fwd_final, h_rev_final)            */
  void* p1;        /* [B, 2h] dtype : saved pre-LayerNorm activations           */
  float* mean;     /* [B]                                                       */
  float* rstd;     /* [B]                                                       */
  void* u;         /* [B, 2h] dtype : saved post-ReLU activations               */
  float* out;      /* [B, h]  fp32                                              */
} tt_head_fwd_io;

int tt_proj_head_fwd(int dtype, const tt_head_fwd_io* io, int ntower, int B, int h, float ln_eps,
                     void* stream);

typedef struct {
  const void* w1; const float* ln_g; const float* ln_b; const void* w2;
  const void* x; const void* p1; const float* mean; const float* rstd; const void* u;
  const float* dout;  /* [B, h] fp32 upstream gradient                              */
  float* dx;          /* [B, 4h] fp32 gradient wrt x                                */
  float* dw1; float* db1; float* dg; float* dbeta; float* dw2; float* db2;  /* fp32 grads (overwritten) */
  void* ws;           /* scratch, tt_proj_head_bwd_ws_size bytes                     */
} tt_head_bwd_io;

int tt_proj_head_bwd(int dtype, const tt_head_bwd_io* io, int ntower, int B, int h, float ln_eps,
                     void* stream);
long tt_proj_head_bwd_ws_size(int dtype, int B, int h);

/* Margin-model head Linear(2H->H) -> LayerNorm(H, eps) -> ReLU -> Dropout(drop_p), one
 * set of weights shared by both towers (margin_two_tower.py:30-35, applied in encode
 * :58-62). Query and doc rows are stacked into one [rows, 2H] batch, so the weight
 * gradients of the backward are already the sum over the two towers. C = H. The dropout
 * mask is the counter-based keep(drop_seed, row, col) of tt_gru_fwd, recomputed by the
 * backward. Weights in dtype (w1 [C, 2C]); biases/LN affine fp32. */
typedef struct {
  const void* x;   /* [rows, 2C] dtype : cat(h_fwd_final, h_rev_final)           */
  const void* w1; const float* b1; const float* ln_g; const float* ln_b;
  void* p1;        /* [rows, C] dtype : saved pre-LayerNorm activations          */
  float* mean;     /* [rows]                                                     */
  float* rstd;     /* [rows]                                                     */
  float* out;      /* [rows, C] fp32                                             */
} tt_head1_fwd_io;

int tt_proj_head1_fwd(int dtype, const tt_head1_fwd_io* io, long rows, int C, float ln_eps, float drop_p,
                      uint32_t drop_seed, void* stream);

typedef struct {
  const void* x; const void* w1; const float* ln_g; const float* ln_b;
  const void* p1; const float* mean; const float* rstd;
  const float* dout;  /* [rows, C] fp32 upstream gradient                          */
  float* dx;          /* [rows, 2C] fp32 gradient wrt x                            */
  float* dw1; float* db1; float* dg; float* dbeta;  /* fp32 grads (overwritten)    */
  void* ws;           /* scratch, tt_proj_head1_bwd_ws_size bytes                  */
} tt_head1_bwd_io;

int tt_proj_head1_bwd(int dtype, const tt_head1_bwd_io* io, long rows, int C, float drop_p, uint32_t drop_seed,
                      void* stream);
long tt_proj_head1_bwd_ws_size(int dtype, long rows, int C);

/* ---------------------------------------------------------------------- losses */
/* y = x / max(||x||_2, eps) row-wise (F.normalize, enhanced_two_tower.py:74-75; also
 * the normalisation inside F.cosine_similarity, :112-117,125-128). y in dtype, y32
 * optional fp32 copy, norm[rows] fp32 = ||x||. */
int tt_l2norm_fwd(int dtype, const float* x, long rows, int cols, float eps, void* y, float* y32,
                  float* norm, void* stream);
/* dx (+)= (dy - y (y.dy)) / max(||x||, eps)  (dy, y32 fp32). */
int tt_l2norm_bwd(const float* dy, const float* y32, const float* norm, long rows, int cols,
                  float eps, float* dx, int accumulate, void* stream);

/* InfoNCE / in-batch softmax cross-entropy over S = inv_tau * qn dn^T
 * (enhanced_two_tower.py:78-82). offdiag_sub is subtracted from every S_ij with
 * j != label_i: the in-batch branch of MarginRankingLoss (:92-101) uses
 * offdiag_sub = margin on un-normalised inputs.
 * Row i's label column is label_offset + i. The B x N score matrix is never written:
 * each workgroup streams dn tiles through one fused MFMA kernel with a running
 * log-sum-exp. Outputs lse[i] and row_loss[i] = lse[i] - S[i][label]. */
int tt_infonce_fwd(int dtype, const void* qn, long bq, const void* dn, long nd, int h,
                   float inv_tau, float offdiag_sub, long label_offset, float* lse,
                   float* row_loss, void* ws, void* stream);
long tt_infonce_fwd_ws_size(long bq, long nd);
/* Gradient of g * sum_i row_loss[i]: dqn [bq,h], ddn [nd,h] (fp32, overwritten).
 * gscale: DEVICE pointer to the fp32 upstream gradient g (autograd's grad_output, read
 * by the kernels so the backward never waits on the host), or NULL for g = 1.
 * ws: tt_infonce_bwd_ws_size bytes; nothing depends on its previous contents.
 * As tt_infonce_fwd, a row of qn / dn must be a multiple of 16 bytes (h % 4 == 0 in fp32,
 * h % 8 == 0 in bf16): any other h, labels outside [0, nd) and (for bq > 0) a null ws are
 * TT_EINVAL before anything is launched. bq = 0 is a no-op. */
int tt_infonce_bwd(int dtype, const void* qn, long bq, const void* dn, long nd, int h,
                   float inv_tau, float offdiag_sub, long label_offset, const float* lse,
                   const float* gscale, float* dqn, float* ddn, void* ws, void* stream);
long tt_infonce_bwd_ws_size(int dtype, long bq, long nd, int h);

/* Symmetric InfoNCE (simple_two_tower.py:73-78): (CE(S, arange) + CE(S^T, arange)) / 2 over
 * the square S = inv_tau * qn dn^T, qn and dn [n, h]; the label of row i is column i and
 * there is no off-diagonal shift. dtype and alignment as tt_infonce_fwd; n = 0 is a no-op.
 * Forward: one pass over the score tiles gives both directions: the running row
 * (max, sum-exp) of tt_infonce_fwd and, per 128-column tile, the (max, sum-exp) of each
 * column over the workgroup's 128 rows, written as one partial per (row block, column)
 * and merged in ascending block order. Outputs lse_row[i] = LSE_j S_ij, lse_col[i] =
 * LSE_j S_ji and row_loss[i] = ((lse_row[i] - S_ii) + (lse_col[i] - S_ii)) / 2.
 * Deterministic: no float atomics, nothing depends on the previous contents of ws
 * (tt_infonce_sym_fwd_ws_size(n, h) bytes). */
int tt_infonce_sym_fwd(int dtype, const void* qn, const void* dn, long n, int h, float inv_tau,
                       float* lse_row, float* lse_col, float* row_loss, void* ws, void* stream);
long tt_infonce_sym_fwd_ws_size(long n, int h);
/* Gradient of g * sum_i row_loss[i]: with
 *   dS_ij = g/2 * (exp(S_ij - lse_row[i]) + exp(S_ij - lse_col[j]) - 2 [i == j]),
 * dqn = inv_tau dS dn and ddn = inv_tau dS^T qn (fp32 [n, h], overwritten). bf16 with h in
 * {128, 256} recomputes the score tiles and never writes dS (the fused backward of
 * tt_infonce_bwd, both LSE vectors read by both roles); every other case, and option
 * infonce_flash = 0, writes dS in dtype and takes two tt_gemm products. gscale as
 * tt_infonce_bwd. ws: tt_infonce_sym_bwd_ws_size bytes. */
int tt_infonce_sym_bwd(int dtype, const void* qn, const void* dn, long n, int h, float inv_tau,
                       const float* lse_row, const float* lse_col, const float* gscale,
                       float* dqn, float* ddn, void* ws, void* stream);
long tt_infonce_sym_bwd_ws_size(int dtype, long n, int h);

/* Group masks: in-batch false negatives. Rows carry row_group[i] and columns col_group[j]
 * (device int32, [bq] and [nd]). THE GROUP RULE, the same in every entry point below:
 *   column j is EXCLUDED for row i  iff
 *     j != label_offset + i  and  row_group[i] >= 0  and  col_group[j] == row_group[i].
 * A negative id is "no group" and excludes nothing; the label column is never excluded.
 * In the softmax losses an excluded entry is absent: it adds nothing to the log-sum-exp,
 * dS_ij = 0, and offdiag_sub does not matter for it. The symmetric loss takes one vector
 * group[n] for both sides (label_offset 0: excl(i, j) iff i != j, group[i] >= 0 and
 * group[i] == group[j]); the same entries are absent from the column LSE.
 * The *_grp entry points are the ungrouped ones with the ids added: the same argument
 * checks before anything is launched, the same workspaces (the same *_ws_size functions,
 * nothing depends on their previous contents), the same kernels with the rule compiled
 * into their tile epilogues. Both id pointers NULL is the ungrouped call, bit for bit (and
 * so are ids that are all negative); exactly one NULL is TT_EINVAL. */
int tt_infonce_fwd_grp(int dtype, const void* qn, long bq, const void* dn, long nd, int h,
                       float inv_tau, float offdiag_sub, long label_offset, const int32_t* row_group,
                       const int32_t* col_group, float* lse, float* row_loss, void* ws, void* stream);
int tt_infonce_bwd_grp(int dtype, const void* qn, long bq, const void* dn, long nd, int h,
                       float inv_tau, float offdiag_sub, long label_offset, const int32_t* row_group,
                       const int32_t* col_group, const float* lse, const float* gscale, float* dqn,
                       float* ddn, void* ws, void* stream);
int tt_infonce_sym_fwd_grp(int dtype, const void* qn, const void* dn, long n, int h, float inv_tau,
                           const int32_t* group, float* lse_row, float* lse_col, float* row_loss,
                           void* ws, void* stream);
int tt_infonce_sym_bwd_grp(int dtype, const void* qn, const void* dn, long n, int h, float inv_tau,
                           const int32_t* group, const float* lse_row, const float* lse_col,
                           const float* gscale, float* dqn, float* ddn, void* ws, void* stream);
/* Mining under the group rule: idx_in [rows, kin] (val_in [rows, kin] optional) are sorted
 * candidate lists, e.g. tt_hardneg_topk's answer for kin = k + g, g the largest number of
 * columns the rule can exclude for one row. Per row the candidates are walked in order and
 * those the rule does not exclude are kept (a candidate outside [0, nd) is dropped too);
 * the first k kept go to idx [rows, k] (and val), nkept[row] = min(kept, k). With fewer
 * than k kept the remaining slots repeat the last kept entry, or column label_offset + row
 * with value -1 when nothing was kept (column 0 when label_offset < 0), so every index
 * written is in [0, nd). An excluded column is never returned; the label column keeps the
 * behaviour of tt_hardneg_topk (it reads as -1 and may be returned once k reaches it).
 * 1 <= k <= kin; label_offset < 0 or label_offset + rows <= nd; the outputs must not
 * overlap the inputs. row_group and col_group are both required. One wave per row, ordered
 * compaction by ballot and prefix count: no atomics. rows = 0 is a no-op. */
int tt_topk_drop_groups(const int32_t* idx_in, const float* val_in, long rows, int kin, long label_offset,
                        const int32_t* row_group, const int32_t* col_group, long nd, int k, int32_t* idx,
                        float* val, int32_t* nkept, void* stream);

/* Hard-negative mining, batched over rows (get_hard_negatives,
 * enhanced_two_tower.py:123-133): sims = qn dn^T (cosine for normalised inputs), the
 * positive column label_offset+i set to -1 (label_offset < 0: no column masked), top-k
 * (1 <= k <= min(tt_topk_max(), nd)) indices per row sorted by descending similarity; ties
 * broken towards the lower column index. Also the scoring step of the serving /search
 * (server/python-api/app.py:94-101, label_offset < 0).
 * idx [bq, k] int32, val [bq, k] fp32 (optional). ws: tt_hardneg_ws_size bytes.
 * k <= 16: bf16 with h in {128, 256, 512} (qn, dn 16-byte aligned, else TT_EINVAL) never stores the
 * score matrix (streamed MFMA scan + exact chunk selection + bit-identical rescoring,
 * tt_score.hip); other shapes store it (tt_gemm) and take a column-split top-k.
 * k > 16: every shape stores the score block (bq * nd * 4 bytes of ws) through tt_gemm and
 * selects with tt_topk_rows. bf16 scores are the same MFMA sums on every path, so a
 * k <= 16 answer is a prefix of a larger-k answer, bit for bit. */
int tt_hardneg_topk(int dtype, const void* qn, long bq, const void* dn, long nd, int h,
                    long label_offset, int k, int32_t* idx, float* val, void* ws, void* stream);
long tt_hardneg_ws_size(int dtype, long bq, long nd, int h, int k);

/* Serving search (server/python-api/app.py:94-101: F.cosine_similarity of one encoded
 * query against every cached document row, then torch.topk): qn [Q, h] fp32 normalised
 * queries, dn [N, h] dtype normalised documents (resident), top-k
 * (1 <= k <= min(tt_topk_max(), N)) indices/scores per query, value descending, ties towards
 * the lower document index. h % 8 == 0. ws: tt_search_ws_size bytes.
 * k <= 16, Q <= 64: one fused pass over dn per 8 queries (per-lane top-k, no score matrix);
 * k <= 16, larger Q: cosine GEMM + column-split top-k.
 * k > 16, any Q: cosine GEMM into the workspace (Q * N * 4 bytes of it), then tt_topk_rows.
 * The scores are then the GEMM's (MFMA sums); the fused scan's are VALU fma chains and can
 * differ from them in the last bit. A k <= 16 answer is therefore guaranteed to be a
 * prefix of a larger-k answer only where both use the GEMM: Q > 64. */
int tt_search_topk(int dtype, const float* qn, long Q, const void* dn, long N, int h, int k,
                   int32_t* idx, float* val, void* ws, void* stream);
long tt_search_ws_size(int dtype, long Q, long N, int h, int k);

/* Int8 document index: one byte per component and one fp32 scale per row.
 *
 * tt_quantize_rows_i8: symmetric per-row quantisation of x [rows, cols] fp32 (leading
 * dimension ld) into codes [rows, cols] int8 (dense) and scale [rows] fp32:
 *   amax = max_c |x[r][c]|;  inv = 127.0f / amax (fp32 division);
 *   codes[r][c] = clamp((int)rintf(x[r][c] * inv), -127, 127)  (fp32 multiply, round half
 *   to even);  scale[r] = amax / 127.0f.
 * A row with amax == 0 gets zero codes and scale 0. cols % 16 == 0, cols <= 1024, ld % 4 == 0,
 * x and codes 16-byte aligned. NaN / infinity inputs are unspecified; rows = 0 is a no-op.
 * One wave per row, one pass. */
int tt_quantize_rows_i8(const float* x, long rows, int cols, long ld, int8_t* codes, float* scale, void* stream);

/* Top-k of every query over an int8 index: qc [Q, h] / qs [Q] the query codes and scales,
 * dc [N, h] / ds [N] the documents' (resident). The score of (query i, document j) is
 *   ((float)dot_ij * ds[j]) * qs[i]
 * with dot_ij the exact int32 dot product of the two code rows and both multiplies fp32, in
 * that order. (float)dot is exact because |dot| <= 127^2 h <= 16 516 096 < 2^24 for
 * h <= 1024: that is why h is capped at 1024. h % 16 == 0, code matrices 16-byte aligned,
 * 1 <= k <= min(tt_topk_max(), N); Q and N limits, ordering (value descending, ties towards
 * the lower document index) and idx / val as tt_search_topk. ws: tt_search_i8_ws_size bytes;
 * nothing depends on its previous contents.
 * k <= 16, few queries: a fused scan (v_dot4_i32_i8, per-lane top-k, no score matrix). By
 *   measurement one pass of it beats the score block and a second pass does not, so by default
 *   it runs for Q <= 4 (k <= 4) and Q <= 2 (k <= 16); option search_i8_qb = n > 0 scans up to
 *   64 queries in groups of at most n, -1 never scans;
 * k <= 16, more queries: an int8 MFMA kernel (v_mfma_i32_32x32x32_i8; a K tail reads as zero
 *   codes) writes the fp32 score block [Q, N] into ws, then the column-split top-k;
 * k > 16, any Q: the same score block, then tt_topk_rows.
 * Every score is an exact integer times two scales, so all three forms return identical
 * bits: a k <= 16 answer is a prefix of any larger-k answer at EVERY Q, and a query's row
 * does not depend on which other queries share the call or on the option (tt_search_topk can
 * promise the prefix only for Q > 64). tt_search_i8_ws_size follows the option's value at
 * the time of the call. */
int tt_search_topk_i8(const int8_t* qc, const float* qs, long Q, const int8_t* dc, const float* ds, long N,
                      int h, int k, int32_t* idx, float* val, void* ws, void* stream);
long tt_search_i8_ws_size(long Q, long N, int h, int k);

/* Second stage of a rescored search, the exact scores of a shortlist:
 *   out[i][r] = qn[i] . dn[cand[i][r]]   (fp32 accumulation),
 * qn [Q, h] fp32, dn [N, h] in dtype (fp32 or bf16), cand [Q, R] int32, out [Q, R] fp32: R
 * rows of dn per query instead of N. A candidate outside [0, N) scores -FLT_MAX.
 * h % 8 == 0, 1 <= R <= 1024, qn and dn 16-byte aligned. One wave per (query, candidate). */
int tt_gather_scores(int dtype, const float* qn, long Q, const void* dn, long N, int h, const int32_t* cand,
                     int R, float* out, void* stream);

/* Largest k of tt_topk_rows, tt_search_topk and tt_hardneg_topk: 1024. */
int tt_topk_max(void);
/* Exact top-k of every row of a dense fp32 block S [rows, cols] (leading dimension ld):
 * idx [rows, k] int32 and val [rows, k] fp32 (optional), 1 <= k <= min(1024, cols), ordered
 * by value descending, ties towards the lower column. Column label_offset + row reads as
 * -1 (label_offset < 0: none) and is returned with that value once k reaches it
 * (enhanced_two_tower.py:130-132). -0.0 and +0.0 are equal and tie by column; infinities
 * and denormals order as floats; val holds the stored values; NaN inputs are unspecified.
 * Radix select of the k-th largest key per (row, column chunk) in LDS, ordered compaction,
 * bitonic sort of the selected; long rows in levels (tt_select.hip). Deterministic: no
 * float atomics, and nothing depends on the previous contents of ws
 * (tt_topk_rows_ws_size(rows, cols, k) bytes; 0 for rows of at most 8192 columns).
 * rows = 0 is a no-op. */
int tt_topk_rows(const float* S, long rows, long cols, long ld, long label_offset, int k,
                 int32_t* idx, float* val, void* ws, void* stream);
long tt_topk_rows_ws_size(long rows, long cols, int k);

/* Full ranks (validate_margin.py:11-54, compute_mrr): the 1-based position of a query's
 * first relevant document among ALL N documents, no top-k cutoff, in two steps so that a
 * corpus can be passed in blocks or shards. qn [Q, h], dn [N, h] dtype rows (cosine for
 * normalised rows), both 16-byte aligned, h % 8 == 0 (else TT_EINVAL).
 *
 * Column j "beats" (theta, t) when s_j > theta, or s_j == theta and j < t: the project's
 * order, value descending and equal scores towards the lower column. -0.0 == +0.0; NaN
 * inputs are unspecified. rank = 1 + #{j beating the best relevant document}.
 *
 * tt_rank_best_relevant: per query the best relevant document, theta[i] = its score and
 * tcol[i] = its column (the largest score over the row's relevant columns, ties to the
 * lowest column); tcol = -1 and theta = 0 for a row without one. Relevance is CSR on the
 * device: rel_ptr [Q + 1] int32 (ascending, rel_ptr[0] the row's first entry), rel_idx
 * int32 columns in [0, N), in any order. The arrays live in device memory, so the host
 * cannot check them: an entry outside [0, N) is skipped, as if it were absent. Every theta
 * is formed with the MFMA instruction, operand orientation and k order of the scan and of
 * tt_gemm, so it has the very bits that tt_rank_count compares against -- document tcol
 * itself and exact duplicates of it land on the right side. ws is unused (may be NULL).
 *
 * tt_rank_count: for each query with tcol >= 0, count[i] = (accumulate ? count[i] : 0) +
 * #{j in [0, N) : column col_offset + j beats (theta[i], tcol[i])}; tcol is a global column,
 * dn holds global columns col_offset .. col_offset + N. A query with tcol < 0 gets 0
 * (accumulate: is left alone). Counting consecutive blocks with accumulate gives exactly
 * the count of one call over the whole matrix: the counts are integers (int32 atomic adds
 * of the column splits' partial counts), so no order of summation changes them, and
 * nothing depends on the previous contents of ws. Q = 0 and N = 0 are no-ops.
 * bf16 with h in {128, 256, 512}: the streamed MFMA scan of tt_hardneg_topk with a counting
 * epilogue, no score is stored. Other shapes, or option rank_gemm = 1: tt_gemm into a row
 * block of ws (at most 1 GiB, rows chunked) and a count over the stored rows; the same
 * counts, bit for bit. ws: tt_rank_count_ws_size bytes. */
int tt_rank_best_relevant(int dtype, const void* qn, long Q, const void* dn, long N, int h,
                          const int32_t* rel_ptr, const int32_t* rel_idx, float* theta, int32_t* tcol,
                          void* ws, void* stream);
int tt_rank_count(int dtype, const void* qn, long Q, const void* dn, long N, int h, long col_offset,
                  const float* theta, const int32_t* tcol, int32_t* count, int accumulate, void* ws,
                  void* stream);
long tt_rank_count_ws_size(int dtype, long Q, long N, int h);

/* Geometry of the streamed score scan (tt_score.hip hn_scan_kernel), host only: nothing is
 * launched and no device memory is touched. Reports what tt_hardneg_topk (what = 0; k as in
 * that call) or tt_rank_count (what = 1; k ignored) would plan for [bq, h] x [nd, h] with the
 * options now in force, from the very functions the launches use:
 *   scan     0 the call does not take the streamed path (other dtype / h, k > 16, option
 *            hn_gemm or rank_gemm, an empty operand): every other field is 0;
 *            1 hn_scan_kernel runs; 2 (what 0, option hn_scan_gemm) the chunk maxima come from
 *            the persistent GEMM instead, the other fields are the plan it shares
 *   variant  hn_scan_v after the fallbacks (0, 4 or 5; 0 for h != 256 and for counts)
 *   rows     query rows per workgroup
 *   map      block map after the map 2 fallback (0, 1 or 2)
 *   nch      64-column tiles of nd;  rt  row tiles;  s  column splits (grid = rt * s)
 *   tps      tiles per split;  last  tiles of the last split (1 <= last <= tps)
 * Tests assert it so that a case written for a tile count keeps reaching it. */
typedef struct tt_scan_geom {
  int scan, variant, rows, map;
  long nch, rt, s, tps, last;
} tt_scan_geom;
int tt_scan_geometry(int what, int dtype, long bq, long nd, int h, int k, tt_scan_geom* out);

/* MarginRankingLoss with explicit negatives (enhanced_two_tower.py:102-121) on
 * normalised vectors: pos_i = qn_i.dn_{label_offset+i}, negm_i = mean_j qn_i.dn_{idx[i,j]},
 * row_loss_i = max(margin - pos_i + negm_i, 0). Negatives are rows of dn. */
int tt_margin_fwd(const float* qn, long bq, const float* dn, long nd, int h, long label_offset,
                  const int32_t* idx, int k, float margin, float* row_loss, void* stream);
/* Gradient of g * sum_i row_loss_i: dqn (overwritten), ddn (accumulated; the caller
 * zeroes it). gscale: device pointer to g (as tt_infonce_bwd) or NULL for 1.
 * ws: tt_margin_bwd_ws_size(bq, nd, h, k) bytes (required). Deterministic: no float
 * atomics; the rows are taken in groups of R (R (k + 1) <= 2048), each group sums the
 * q rows of each document it mined in entry order, and each document's group partials
 * are added in ascending group order (hard negatives are shared by many rows).
 * 1 <= k < 2048. */
int tt_margin_bwd(const float* qn, long bq, const float* dn, long nd, int h, long label_offset,
                  const int32_t* idx, int k, float margin, const float* gscale, float* dqn, float* ddn,
                  void* ws, void* stream);
long tt_margin_bwd_ws_size(long bq, long nd, int h, int k);

/* out[0] = scale * sum_i x[i]. */
int tt_sum(const float* x, long n, float scale, float* out, void* stream);

/* ------------------------------------------------------------------- optimiser */
/* torch.optim.Adam (train_enhanced.py:43,63) over up to 48 fp32 tensors per call,
 * bit-for-bit the update order of torch's single-tensor Adam:
 *   m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2 ;
 *   p -= lr/(1-b1^step) * m / (sqrt(v)/sqrt(1-b2^step) + eps)   (g += wd*p first).
 * skip: device int32 word or NULL; when it reads non-zero at launch time the kernel
 * changes nothing (p, m, v untouched). two_towers_amd.Adam passes the OR of the status
 * words of the column-split forwards since the last step (tt_gru_fwd ws), so a step whose
 * forward timed out cannot update the weights; no host synchronisation is involved. */
int tt_adam_multi(float* const* params, const float* const* grads, float* const* exp_avg,
                  float* const* exp_avg_sq, const long* sizes, int ntensors, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int step, const int32_t* skip, void* stream);
/* torch.optim.AdamW (simple_two_tower.py:193), same parameters: decoupled decay in the
 * order of torch's single-tensor AdamW, p *= (float)(1 - (double)lr * weight_decay) first,
 * then the Adam update above with g untouched. skip as tt_adam_multi. */
int tt_adamw_multi(float* const* params, const float* const* grads, float* const* exp_avg,
                   float* const* exp_avg_sq, const long* sizes, int ntensors, float lr, float beta1,
                   float beta2, float eps, float weight_decay, int step, const int32_t* skip, void* stream);

/* sumsq[0] = (accumulate ? sumsq[0] : 0) + sum of g^2 over up to 48 fp32 tensors (device
 * scalar); more tensors chain through accumulate. One fp32 partial per 4096-element chunk
 * of the concatenated tensors, then one workgroup adds the partials in a fixed order:
 * the same inputs give the same bits. ws: tt_grad_norm_ws_size(sizes, ntensors) bytes. */
int tt_grad_norm_multi(const float* const* grads, const long* sizes, int ntensors, int accumulate,
                       float* sumsq, void* ws, void* stream);
long tt_grad_norm_ws_size(const long* sizes, int ntensors);
/* torch.nn.utils.clip_grad_norm_ (simple_two_tower.py:239), every value computed on the
 * device: total = sqrt(sumsq[0]), coef = min(1, max_norm / (total + 1e-6)), g *= coef for
 * up to 48 tensors; total_norm_out[0] = total (optional). A non-finite norm propagates
 * into the gradients as with error_if_nonfinite=False. */
int tt_clip_scale_multi(float* const* grads, const long* sizes, int ntensors, const float* sumsq,
                        float max_norm, float* total_norm_out, void* stream);

/* ------------------------------------------------------- trainable embedding table */
/* Segment sum of gradient rows by token id: rows[u, :] = sum of dx[perm[p], 0:e] over
 * seg_ptr[u] <= p < seg_ptr[u+1], p ascending. dx fp32 [n, ldx] (the layer-0 data gradient,
 * one row per token position); perm int32 [m]: the row numbers of dx ordered by token id
 * (stable, pads removed); seg_ptr int32 [nseg + 1], strictly increasing from 0 to m: one
 * segment per distinct id; rows fp32 [nseg, e], every row written whole (overwritten).
 * A perm entry outside [0, n) adds nothing.
 *  - fp32 accumulation, no float atomics;
 *  - every element is a sum in an order fixed by (perm, seg_ptr) alone: workgroup k adds the
 *    positions [k C, (k+1) C) (C = tt_embed_grad_chunk()) of each segment in order, and a
 *    segment that reaches into several chunks is the sum of its per-chunk partials in chunk
 *    order (second launch). Two calls give the same bits;
 *  - ws: tt_embed_grad_ws_size(m, e) bytes holding those partials; only slots written by
 *    the call are read, so nothing depends on its previous contents;
 *  - nseg = 0, m = 0 and n = 0 are no-ops;
 *  - any e >= 1: 16-byte loads when e % 4 == 0, ldx % 4 == 0 and dx, rows, ws are 16-byte
 *    aligned, else a scalar path with the same sums. n, m < 2^31. */
int tt_embed_grad_rows(const float* dx, long n, long ldx, const int32_t* perm, long m,
                       const int32_t* seg_ptr, long nseg, int e, float* rows, void* ws, void* stream);
long tt_embed_grad_ws_size(long m, int e);
/* Sorted positions per workgroup of tt_embed_grad_rows (the chunk size C above). */
int tt_embed_grad_chunk(void);
/* tt_embed_grad_rows with the row of segment u placed at rows[dst[u]] of a larger buffer:
 * the data-parallel form, where dst[u] is the position of this rank's u-th id in the union of
 * all ranks' ids and the [nrows, e] buffers of the ranks are then summed by one all-reduce.
 * dst int32 [nseg], strictly ascending; rows fp32 [nrows, e], nrows >= nseg. A dst[u] outside
 * [0, nrows) drops that segment.
 *  - every row of rows is written by the call, each element once: the rows no segment names
 *    are +0.0f (also with nseg = 0, m = 0 or n = 0 while nrows > 0), so the caller clears
 *    nothing; nrows = 0 is a no-op;
 *  - the sums are the bits tt_embed_grad_rows gives for the same (dx, perm, seg_ptr): the
 *    same chunks, the same order inside a chunk and across chunks; no float atomics;
 *  - ws: tt_embed_grad_ws_size(m, e) bytes, as above;
 *  - 16-byte accesses under the same rule as above (e % 4 == 0, ldx % 4 == 0, dx, rows, ws
 *    16-byte aligned), else the scalar path. n, m, nrows < 2^31. */
int tt_embed_grad_rows_at(const float* dx, long n, long ldx, const int32_t* perm, long m,
                          const int32_t* seg_ptr, long nseg, const int32_t* dst, long nrows,
                          int e, float* rows, void* ws, void* stream);

/* torch.optim.SparseAdam's step (torch/optim/_functional.py sparse_adam) on the rows
 * ids[0..nrows) (distinct, int32) of weight / exp_avg / exp_avg_sq (fp32 [vocab, e]) with
 * the summed gradient rows (fp32 [nrows, e]):
 *   dm = (g - m)(1-b1); dv = (g^2 - v)(1-b2); m += dm; v += dv;
 *   w -= lr sqrt(1-b2^step)/(1-b1^step) * (m / (sqrt(v) + eps))
 * (eps joins sqrt(v) before the bias corrections, which use the global step: not dense
 * Adam's formula). Rows not named by ids are neither read nor written (lazy moments); an id
 * outside [0, vocab) is skipped. copy (optional): the [vocab, ep] copy of weight in
 * copy_dtype that tt_embed_gather reads; columns [0, e) of the touched rows are rewritten
 * from the new fp32 values (round-to-nearest-even for bf16), columns e.. are left alone.
 * skip as tt_adam_multi: non-zero at launch time means nothing changes. */
int tt_sparse_adam_rows(float* weight, float* exp_avg, float* exp_avg_sq, long vocab, int e,
                        const int32_t* ids, const float* rows, long nrows, int copy_dtype, void* copy,
                        int ep, float lr, float beta1, float beta2, float eps, int step,
                        const int32_t* skip, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TT_HIP_H */
