/* polypmae.h -- C-ABI of the MI355X (gfx950) hot path for SSL4POLYP's MAE pre-train /
 * ViT-B/16 fine-tune step.
 *
 * The reference (irconde/SSL4POLYP) has no FFI of its own: its hot path is the torch/timm op
 * sequence inside MaskedAutoencoderViT.forward (src/ssl4polyp/models/mae/models_mae.py:150-220),
 * ViT_from_MAE.forward / VisionTransformer_from_Any.forward (src/ssl4polyp/models/models.py:117-140,
 * 196-222) and autograd's backward of them (train_classification.py:4531-4533,
 * mae/engine_pretrain.py:52-65).  Each entry point below names the reference op(s) it replaces.
 *
 * Conventions
 *   - plain pointers + sizes; every pointer is DEVICE memory owned by the caller; the library never
 *     allocates, frees, retains pointers or synchronises; every launch goes to `stream`
 *     (a hipStream_t passed as void*).
 *   - return 0 on success, negative pm_status otherwise; no C++ exceptions cross the ABI.
 *   - dtype codes: PM_F32 = 0, PM_BF16 = 1, PM_F16 = 2.  "act" tensors (activations between kernels) use the
 *     precision mode's activation type: bf16 in PM_BF16 mode, IEEE half in PM_F16 mode, f32 in PM_F32 mode.
 *     PM_F16 is the reference's own AMP arithmetic (torch.cuda.amp.autocast runs every matmul in fp16 with f32
 *     accumulation: train_classification.py:4527-4546, engine_pretrain.py:52): same kernels, same MFMA rate
 *     (v_mfma_f32_32x32x16_f16), 11 significant bits per operand instead of 8.  The backward operands are fp16 too
 *     (an MFMA takes one type for both operands), so the caller scales the loss as the reference's GradScaler does;
 *     every backward entry point is linear in its incoming gradient and passes inf / nan through.
 *   - matrices are row-major with explicit leading dimensions in ELEMENTS.
 */
#ifndef POLYPMAE_H
#define POLYPMAE_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum pm_status { PM_OK = 0, PM_EINVAL = -1, PM_ESHAPE = -2, PM_EARCH = -3, PM_ELAUNCH = -4, PM_EALIGN = -5 };
enum pm_dtype { PM_F32 = 0, PM_BF16 = 1, PM_F16 = 2 };

/* epilogue selector of pm_gemm (what happens to acc = op(A)*op(B) before it is stored) */
enum pm_epilogue {
  PM_EPI_STORE = 0,      /* C = acc (+bias)                                          (any Linear) */
  PM_EPI_GELU = 1,       /* aux = acc+bias (pre-activation; aux NULL: not stored), C = gelu_erf(acc+bias)  (timm Mlp.fc1 + act) */
  PM_EPI_RESIDUAL = 2,   /* C_f32 = resid_f32 + acc + bias                           (Block residual adds) */
  PM_EPI_DGELU = 3,      /* C = acc * gelu_erf'(aux)                                 (backward of Mlp.act) */
  PM_EPI_ACCUM = 4       /* C_f32 += acc                                             (grad accumulation) */
};

const char* pm_strerror(int status);
int pm_abi_version(void);

/* LayerNorm(eps) over the last dim -- replaces nn.LayerNorm in timm Block.norm1/norm2,
 * MaskedAutoencoderViT.norm / decoder_norm (models_mae.py:42,57,168,188).
 * x: f32 [M, D] with row stride ldx; y: out_dtype [M, D] contiguous; mean/rstd: f32 [M] (saved for backward).
 * D <= 1280 (ViT-H), D % 4 == 0. */
int pm_layernorm_fwd(const float* x, long ldx, const float* gamma, const float* beta, void* y, int out_dtype,
                     float* mean, float* rstd, int M, int D, float eps, void* stream);

/* Backward of the above fused with the residual-gradient add of the pre-LN block
 * (x_out = x + f(LN(x)) => dx = dres + LN'(dy)):
 *   dx_f32[M,D] (ld ldx) = (dres ? dres : 0) + LN_bwd(dy);  dx_act (optional) = cast(dx_f32)
 *   dgamma += sum_m dy*xhat ; dbeta += sum_m dy ; dcolsum (optional) += sum_m dx   (bias grad of the
 *   Linear whose output was added into this residual stream).  The three accumulators must be
 *   zero-initialised (or hold the running gradient) by the caller.  `workspace` (>= 512*3*D*4 bytes, optional):
 *   per-block partial column sums, reduced in a fixed order by a second launch; without it the sums use
 *   float atomics (order-dependent rounding). */
int pm_layernorm_bwd(const void* dy, int dy_dtype, const float* x, long ldx, const float* gamma, const float* mean,
                     const float* rstd, const float* dres, long lddres, float* dx, long lddx, void* dx_act,
                     int act_dtype, float* dgamma, float* dbeta, float* dcolsum, int M, int D, void* workspace,
                     size_t ws_bytes, void* stream);

/* General matrix product with fused epilogue -- replaces every nn.Linear / Conv2d-as-GEMM of the path
 * and their dgrad / wgrad.   acc[M,N] = sum_k A(m,k) * B(n,k)
 *   a_kmajor = 0: A stored [M][K] (lda);  1: A stored [K][M] (lda)   (wgrad: A = dY^T)
 *   b_kmajor = 0: B stored [N][K] (ldb);  1: B stored [K][N] (ldb)   (dgrad: B = W as stored; wgrad: B = X)
 * in_dtype: element type of A and B (PM_BF16 -> v_mfma_f32_32x32x16_bf16, PM_F32 -> v_mfma_f32_32x32x2_f32).
 * bias: f32 [N] or NULL.  C: c_dtype [M][N] (ldc).  aux: in_dtype [M][N] (ldc) for GELU / DGELU.
 * resid: f32 [M][N] (ldc) for PM_EPI_RESIDUAL (may alias C). */
int pm_gemm(const void* A, long lda, int a_kmajor, const void* B, long ldb, int b_kmajor, int in_dtype,
            const float* bias, void* C, long ldc, int c_dtype, int epilogue, void* aux, const float* resid,
            int M, int N, int K, void* stream);

/* Same as pm_gemm with a caller-owned scratch buffer: when the output has few 128x128 tiles and K is long (the wgrad
 * shapes: K = number of tokens) the k-loop is split over up to 16 blocks per tile, partial sums go to f32 slabs in
 * `workspace` and are reduced in a fixed order (deterministic).  ws_bytes >= 16*M*N*4 enables every split. */
int pm_gemm_ws(const void* A, long lda, int a_kmajor, const void* B, long ldb, int b_kmajor, int in_dtype,
               const float* bias, void* C, long ldc, int c_dtype, int epilogue, void* aux, const float* resid,
               int M, int N, int K, void* workspace, size_t ws_bytes, void* stream);

/* pm_gemm_ws with per-call options (no process-wide tuning state):
 *   max_blocks: workgroups a split-K weight-gradient GEMM (both operands k-major) spreads over; 0 = 256 = the whole
 *               chip (fastest alone).  A caller that runs weight gradients on a second stream beside the dgrad chain
 *               passes ~128 so that the chain keeps half of the CUs (the training engine does: +4.5 % step rate).
 *   variant:    the one per-call override of the kernel choice (tests, tuning scripts); it names shipped kernels only.
 *               Bits 0-5: 0 = the dispatcher's heuristics; 1 = the 128x128 kernels; 8, 9, 10, 24, 25, 26 = that ring-kernel
 *               configuration for a problem that fits the ring kernel (16-bit operands, A k-normal, K % 32 == 0,
 *               M >= 1024) -- this also switches the few-tiles rule off.  Bits 6-7: tile of a ring weight gradient (both
 *               operands k-major), 0 = heuristics, 1 = 256x128, 2 = 256x256.  Any other value, or a ring configuration
 *               that is not built for the call's B layout (9, 10, 25, 26 exist for k-normal B only), returns PM_EINVAL.
 *               The values are not stable across ABI versions. */
typedef struct pm_gemm_opts {
  int max_blocks;
  int variant;
} pm_gemm_opts;
int pm_gemm_ex(const void* A, long lda, int a_kmajor, const void* B, long ldb, int b_kmajor, int in_dtype,
               const float* bias, void* C, long ldc, int c_dtype, int epilogue, void* aux, const float* resid,
               int M, int N, int K, void* workspace, size_t ws_bytes, const pm_gemm_opts* opts, void* stream);

/* The dispatcher's plan for a GEMM WITHOUT launching: returns the status pm_gemm_ex would return for these layouts, types,
 * shapes and options (PM_OK, PM_ESHAPE, PM_EALIGN, PM_EINVAL; pointers and leading dimensions are not seen, so their
 * checks are not made) and, when PM_OK, fills *info.  has_bias: bias != NULL; ldc_is_n: ldc == N; ws_bytes: the scratch
 * the call would pass (0 = none).  A host engine or a test uses it to know which kernel a Linear runs on. */
#define PM_GEMM_GENERIC 0    /* 128x128, register-staged, any K % chunk == 0 */
#define PM_GEMM_LDS128 1     /* 128x128, LDS-DMA, optional split-K */
#define PM_GEMM_RING 2       /* large-tile ring kernel (forward / dgrad) */
#define PM_GEMM_RING_WGRAD 3 /* large-tile ring kernel, both operands k-major, split-K */
typedef struct pm_gemm_plan_info {
  int family;        /* PM_GEMM_* */
  int cfg;           /* ring configuration (pm_gemm_opts.variant bits 0-5), 0 for the other families */
  int tile_m, tile_n;
  int split_k;       /* k-slices (1 = none); > 1: f32 slabs in the workspace and a reduce launch */
  int band;          /* PM_GEMM_RING: tile columns per band of the tile order (0 = row by row) */
  size_t ws_bytes;   /* scratch the plan uses */
} pm_gemm_plan_info;
int pm_gemm_plan(int a_kmajor, int b_kmajor, int in_dtype, int has_bias, int c_dtype, int ldc_is_n, int epilogue, int M, int N,
                 int K, size_t ws_bytes, const pm_gemm_opts* opts, pm_gemm_plan_info* info);

/* Every weight gradient of one transformer block in ONE launch (autograd of timm Block's four Linears: attn.qkv,
 * attn.proj, mlp.fc1, mlp.fc2 -- models_mae.py:39-41,53-55 through engine_pretrain.py:65 / tc.py:4533):
 *   dW_i[n_out][n_in] (+)= dY_i^T X_i,   dY_i act [K][n_out] (lddy), X_i act [K][n_in] (ldx), K = number of tokens.
 * The weight gradients have a huge reduction dimension and few output tiles; one GEMM at a time needs split-K (short
 * k-loops, f32 slabs, a reduce launch each).  Grouped, the ~100 tiles of a ViT-B block each run their whole K in one
 * workgroup: no slabs, no reduce, deterministic, and the launch occupies ~100 CUs beside the caller's dgrad chain.
 * `items` is a HOST array of n <= 8 descriptors (copied into the kernel arguments).  Returns PM_ESHAPE when the group
 * does not fit the ring kernel (f32 mode, K % 32 != 0, K < 2048, n_out < 256, n_in < 128): the caller then issues
 * pm_gemm_ws per gradient. */
typedef struct pm_wgrad_item {
  const void* dY;
  long lddy;
  const void* X;
  long ldx;
  float* dW;
  long lddw;
  int n_out, n_in;
  int accumulate; /* dW += (gradient accumulation) instead of dW = */
  float* dbias;   /* optional f32 [n_out]: += column sums of dY = the Linear's bias gradient, computed beside the GEMM on
                     the matrix cores (the dY fragments are already in registers) instead of by a separate pm_colsum pass */
} pm_wgrad_item;
/* max_blocks: workgroups (= CUs) the launch may occupy; 0 = one per work item.  Fewer workgroups walk several items each.
 * A group with fewer than 64 tiles of 256x256 and a long K (the 512-wide MAE decoder block: 48 tiles, K = 50 432 tokens)
 * is cut into k-slices so that tiles x slices fills the chip (48 x 4): f32 partials go to `workspace`
 * (pm_wgrad_group_workspace_bytes; 16-byte aligned) and ONE reduce launch on the same stream finishes every dW / dbias of
 * the group in a fixed order.  With workspace == NULL (or too small) such a group runs whole-K tiles of 256x128 instead.
 * max_blocks == PM_GROUP_WHOLE_K: never slice, whole-K tiles of 256x256 whatever the tile count -- for a caller that runs
 * this group beside another launch of the same kind (pm_vit_block_bwd's second group) and fills the chip that way. */
#define PM_GROUP_WHOLE_K (-1)
int pm_wgrad_group(const pm_wgrad_item* items, int n, int K, int in_dtype, int max_blocks, void* workspace, size_t ws_bytes,
                   void* stream);
size_t pm_wgrad_group_workspace_bytes(const pm_wgrad_item* items, int n, int K, int in_dtype);
/* Admission test and plan of pm_wgrad_group WITHOUT launching: returns the status pm_wgrad_group would return for these
 * shapes / alignments (PM_OK, PM_ESHAPE, PM_EALIGN, PM_EINVAL) and, when PM_OK, the scratch it wants (*ws_bytes), the number
 * of 256x256 output tiles of the group (*tiles256) and the k-slices per tile (*k_slices; 1 = whole-K tiles, no slabs).  The
 * pointers of the items are only checked for NULL / alignment.  pm_vit_block_bwd runs this before its first launch; a host
 * engine uses it instead of restating the rules. */
int pm_wgrad_group_plan(const pm_wgrad_item* items, int n, int K, int in_dtype, size_t* ws_bytes, int* tiles256,
                        int* k_slices);

/* Fused multi-head self-attention core -- replaces timm Attention.forward between qkv and proj:
 * softmax(q k^T * dh^-0.5) v, never materialising the [N,N] scores in HBM.
 * qkv: act [B, N, 3, H, dh] (the qkv Linear's output as stored); out: act [B, N, H*dh];
 * lse: f32 [B, H, N] (log-sum-exp of the scaled scores, saved for backward).
 * Supported: dh in {32, 64, 80} (ViT-B / MAE decoder / ViT-H), N <= 288 (257 = patch 14 at 224^2). */
int pm_attention_fwd(const void* qkv, void* out, float* lse, int B, int N, int H, int dh, int dtype, void* stream);
/* Backward: dqkv [B,N,3,H,dh] from dout [B,N,H*dh]; delta: f32 workspace [B,H,N]. */
int pm_attention_bwd(const void* qkv, const void* out, const void* dout, const float* lse, float* delta, void* dqkv,
                     int B, int N, int H, int dh, int dtype, void* stream);

/* What pm_attention_fwd / pm_attention_bwd launch for a shape, WITHOUT launching: returns the status they would return
 * (PM_OK, PM_ESHAPE, PM_EINVAL; pointers are not seen) and, when PM_OK, fills *info. */
#define PM_ATTN_FWD_HEAD 0        /* forward, one workgroup per (batch, head) */
#define PM_ATTN_FWD_PERSISTENT 1  /* forward, a workgroup walks several heads, the next one's K / V / Q in flight */
#define PM_ATTN_BWD_SPLIT 2       /* backward, query-side and key-side kernels (two launches; delta is their hand-over) */
#define PM_ATTN_BWD_FUSED 3       /* backward, dQ, dK and dV of a head from one set of LDS images */
typedef struct pm_attention_plan_info {
  int family;          /* PM_ATTN_* */
  int nt;              /* 32-token tiles of the instantiated kernel = waves per workgroup */
  int ct;              /* tiles an LDS image holds at a time (== nt: the head is staged once) */
  int grid;            /* workgroups per launch */
  int launches;
  size_t lds_bytes[2]; /* dynamic LDS of each launch */
} pm_attention_plan_info;
int pm_attention_plan(int backward, int B, int N, int H, int dh, int dtype, pm_attention_plan_info* info);

/* Column sums of a [M,N] act matrix into f32 [N] (+=) -- bias gradients of qkv / fc1 / decoder Linears. */
int pm_colsum(const void* x, long ldx, int dtype, float* out, int M, int N, void* stream);
/* Deterministic form: per-split partial rows go to `workspace` (>= 128*N*4 bytes) and are summed in a fixed order;
 * without a workspace the splits are combined with float atomics (order-dependent last bits). */
int pm_colsum_ws(const void* x, long ldx, int dtype, float* out, int M, int N, void* workspace, size_t ws_bytes,
                 void* stream);

/* Patch extraction (the im2col of timm PatchEmbed's Conv2d k=s=p), optionally only the kept patches
 * of MAE random masking (models_mae.py:141-142 applied BEFORE the projection, which is the same
 * linear map per patch): imgs f32 [B,C,Himg,Himg] NCHW -> cols act [B*keep, ldcols], the first C*p*p of a row in (c,py,px)
 * order, the rest zero (ldcols > C*p*p: the reduction dimension padded to the GEMM's k-step -- 3*14*14 = 588 -> 640 for
 * mae_vit_huge_patch14, models_mae.py:239-244).  Any p that divides img (16-B reads when p % 4 == 0).
 * ids_keep: int32 [B, keep] patch indices, or NULL for all patches in raster order (keep = L). */
int pm_patch_im2col(const float* imgs, const int* ids_keep, void* cols, long ldcols, int out_dtype, int B, int C, int img,
                    int p, int keep, void* stream);

/* Zero-padded operand copy and its inverse, for a Linear whose reduction dimension is not a multiple of the matrix-core
 * kernels' 16-byte chunks (patch 14: PatchEmbed.proj [D, 588], decoder_pred [588, Dd]; models_mae.py:36,57):
 *   pm_pad_cast : dst act [rows_pad, ldd] <- src f32 [rows, lds] in the top-left corner, zeros elsewhere (up to cols_pad)
 *   pm_unpad_add: dst f32 [rows, ldd] (+)= src f32 [rows, lds], the first `cols` columns (the valid part of a gradient
 *                 computed in the padded layout; accumulate = 0 stores). */
int pm_pad_cast(const float* src, long lds, void* dst, long ldd, int dst_dtype, int rows, int cols, int rows_pad,
                int cols_pad, void* stream);
int pm_unpad_add(const float* src, long lds, float* dst, long ldd, int rows, int cols, int accumulate, void* stream);

/* Token assembly: x[b,0,:] = cls + pos[0]; x[b,1+j,:] = emb[b*keep+j,:] + pos[1+id(b,j),:]
 * (models_mae.py:155-163; models.py:198-201 / 28-33).  emb f32 [B*keep, D]; x f32 [B, 1+keep, D]. */
int pm_assemble_tokens(const float* emb, const float* cls, const float* pos, const int* ids_keep, float* x,
                       int B, int keep, int D, void* stream);
/* Backward: demb[b*keep+j] = dx[b,1+j]; dcls (optional) += sum_b dx[b,0]; dpos (optional, learnable pos_embed)
 * += scatter of dx, row 0 (the cls position) included whether or not dcls is given.  demb act-typed [B*keep, D]. */
int pm_assemble_tokens_bwd(const float* dx, const int* ids_keep, void* demb, int act_dtype, float* dcls, float* dpos,
                           int B, int keep, int D, void* stream);

/* MAE random masking from noise (models_mae.py:123-148): stable ascending argsort per sample.
 * noise f32 [B,L]; ids_shuffle/ids_restore int32 [B,L]; mask f32 [B,L] (1 = removed). L <= 1024. */
/* Masking noise for random_masking (models_mae.py:132 `torch.rand(N, L, device=x.device)`): noise[i] = U[0, 1) with 24 random bits,
 * Philox4x32-10 keyed by `seed`, counter = (i / 4, stream_id) -- a pure function of (seed, stream_id, i), whatever the launch
 * geometry, device or rank layout.  The caller advances stream_id per draw (per forward pass). */
int pm_mae_noise(float* noise, long n, unsigned long long seed, unsigned int stream_id, void* stream);
int pm_mae_masking(const float* noise, int* ids_shuffle, int* ids_restore, float* mask, int B, int L, int len_keep,
                   void* stream);

/* MAE decoder input (models_mae.py:177-183): mask-token fill + unshuffle + cls re-attach + pos add.
 * emb f32 [B, 1+keep, D]; out f32 [B, 1+L, D]. */
int pm_mae_unshuffle(const float* emb, const float* mask_token, const float* dpos, const int* ids_restore, float* out,
                     int B, int L, int keep, int D, void* stream);
/* Backward: demb act-typed [B,1+keep,D] (pure gather through ids_shuffle); dmask_token f32 [D] (+=).
 * workspace (pm_workspace_bytes(PM_WS_UNSHUFFLE_BWD, M, D) = 1024*D*4 bytes) makes the mask-token sum two-stage and deterministic;
 * NULL (or less than rows*D*4 for the launch's block rows) falls back to float atomics. */
int pm_mae_unshuffle_bwd(const float* dout, const int* ids_shuffle, void* demb, int act_dtype, float* dmask_token,
                         int B, int L, int keep, int D, void* workspace, size_t ws_bytes, void* stream);

/* MAE reconstruction loss (models_mae.py:95-107,198-214): fused patchify + (optional norm_pix) + per-patch MSE.
 * pred f32 rows of `ldp` elements (ldp >= p*p*C, a multiple of 4; anything else: PM_ESHAPE); row (b*(L+1)+1+l) holds patch l of sample b when has_cls_row=1 (the
 * decoder_pred output incl. the cls row), row b*L+l otherwise.  patch_loss f32 [B*L] = mean((pred-target)^2, -1).
 * pm_mae_loss_finish reduces deterministically (single block): sums = {sum(loss*mask), sum(mask)},
 * loss = sums[0]/sums[1]  (models_mae.py:213). */
int pm_mae_loss_fwd(const float* imgs, const float* pred, long ldp, int has_cls_row, float* patch_loss, int B, int C,
                    int img, int p, int norm_pix, void* stream);
int pm_mae_loss_finish(const float* patch_loss, const float* mask, long n, float* sums, float* loss, void* stream);
/* Backward: dpred act-typed [B*(L+has_cls_row), lddp] (lddp >= p*p*C, a multiple of 4; columns beyond p*p*C zeroed;
 * ldp < p*p*C or lddp < p*p*C: PM_ESHAPE), same row order as pred (cls rows and kept patches zeroed); dloss f32 scalar on device. */
int pm_mae_loss_bwd(const float* imgs, const float* pred, long ldp, int has_cls_row, const float* mask,
                    const float* sums, const float* dloss, void* dpred, long lddp, int act_dtype, int B, int C, int img,
                    int p, int norm_pix, void* stream);

/* Rows of a [*, row_bytes] array by index, and back into an all-zero array (engine: the classifier's top block under out_token
 * "cls" -- models.py:134-136 -- whose incoming gradient lives in one row per sample):
 *   pm_gather_rows      : dst[r] = src[idx[r]] for r < R          (row_bytes % 4 == 0; source row pitch ld_bytes)
 *   pm_scatter_rows_zero: dst[m] = inv[m] >= 0 ? src[inv[m]] : 0  for m < M   (row_bytes % 16 == 0, 16-byte aligned buffers) */
int pm_gather_rows(const void* src, long ld_bytes, const int* idx, void* dst, int R, long row_bytes, void* stream);
int pm_scatter_rows_zero(const void* src, const int* inv, void* dst, int M, long row_bytes, void* stream);

/* f32 -> act cast (weight shadow copies for the bf16 MFMA path). */
int pm_cast(const float* src, void* dst, int dst_dtype, long n, void* stream);

/* Device-side tail of the input pipeline -- replaces torchvision `ToTensor()` + `Normalize(mean, std)`
 * and the two random flips of the reference's transform (classification/data/transforms.py:225-253) on frames that
 * arrive as decoded uint8: src u8 [B][H][W][3] (HWC, what PIL / numpy hold), dst f32 [B][3][H][W].
 *   dst = (float(src) / 255 - mean[c]) / std[c]   (same operations, same order, IEEE f32: bit-exact with torchvision)
 * flip_flags: u8 [B] or NULL; bit 0 = horizontal flip, bit 1 = vertical flip of that sample.  W % 4 == 0.
 * A uint8 batch is a quarter of the f32 batch on PCIe (9.6 MB instead of 38.5 MB at B = 64). */
int pm_preprocess_u8(const unsigned char* src, const unsigned char* flip_flags, float* dst, int B, int H, int W,
                     float mean_r, float mean_g, float mean_b, float std_r, float std_g, float std_b, void* stream);

/* ---- train-time augmentation on the device (classification/data/transforms.py:234-246) ----------------
 * The reference applies Resize, ColorJitter(0.4, 0.5, 0.25, 0.01), GaussianBlur((25, 25), sigma in [0.001, 2]), two random flips
 * and RandomRotation(180) per image in PIL / torchvision 0.10 on DataLoader workers.  These entry points do the same work on
 * uint8 HWC frames [B][H][W][3] resident in HBM, with the arithmetic of the library routines the reference ends up in (Pillow
 * Resample.c 8bpc, Blend.c, Convert.c rgb2l / rgb2hsv / hsv2rgb, Geometry.c affine_fixed; torchvision's tensor gaussian_blur):
 * results equal oracle/augment_ref.py bit for bit, which is pinned against Pillow itself.  Random parameters are the caller's. */

/* Resize (Image.resize(BILINEAR), antialiased): horizontal then vertical pass with Pillow's 22-bit fixed-point taps, which the
 * caller builds as Resample.c precompute_coeffs + normalize_coeffs_8bpc do: bounds_* i32 [out][2] = (first source index, count),
 * taps_* i32 [out][ksize].  tmp u8 [B][Hs][Wo][3] (needed when both sizes change).  A pass whose size does not change is skipped. */
int pm_aug_resize_u8(const unsigned char* src, unsigned char* tmp, unsigned char* dst, const int* bounds_x, const int* taps_x,
                     int ksize_x, const int* bounds_y, const int* taps_y, int ksize_y, int B, int Hs, int Ws, int Ho, int Wo,
                     void* stream);

/* RandomResizedCrop's arithmetic (mae/main_pretrain.py:157: RandomResizedCrop(224, scale=(0.2, 1.0), interpolation=bicubic) ->
 * functional.resized_crop = img.crop(box).resize((out, out), BICUBIC)): every sample has its own crop box = (top, left, h, w)
 * (i32 [B][4], inside the frame, drawn by the caller) and therefore its own resample taps, which are built ON THE DEVICE in the
 * double arithmetic of Resample.c (two small launches), followed by the horizontal and the vertical pass.  bicubic = 0 uses the
 * bilinear filter.  workspace: pm_aug_resized_crop_workspace_bytes(B, Hs, Ws, out) bytes, 16-byte aligned. */
size_t pm_aug_resized_crop_workspace_bytes(int B, int Hs, int Ws, int out);
int pm_aug_resized_crop_u8(const unsigned char* src, const int* box, unsigned char* dst, int bicubic, int B, int Hs, int Ws, int out,
                           void* workspace, size_t ws_bytes, void* stream);
/* The same over a packed ragged batch (frames of different decoded sizes, as an image folder holds them): frame b is HWC uint8 of
 * hw[b] = (H_b, W_b) (i32 [B][2]) starting at byte offset[b] (i64 [B]) of src; box[b] lies inside frame b; H_b <= Hmax, W_b <= Wmax.
 * dst [B][out][out][3].  Same arithmetic and the same kernels as pm_aug_resized_crop_u8 (which is this call with uniform frames);
 * workspace: pm_aug_resized_crop_workspace_bytes(B, Hmax, Wmax, out) bytes, 16-byte aligned.  The tables are device memory and are
 * not validated here (the caller checks them before the upload).  B <= 65535. */
int pm_aug_resized_crop_ragged_u8(const unsigned char* src, const long long* offset, const int* hw, const int* box, unsigned char* dst,
                                  int bicubic, int B, int Hmax, int Wmax, int out, void* workspace, size_t ws_bytes, void* stream);

/* The validation transform of the MAE recipes (mae/main_linprobe.py:151-156: Resize(resize, bicubic) + CenterCrop(crop)) over the
 * packed ragged batch of pm_aug_resized_crop_ragged_u8 (src, offset i64 [B], hw i32 [B][2]): dst u8 [B][crop][crop][3] equals
 * Image.resize((nw, nh), BICUBIC).crop((left, top, left + crop, top + crop)) byte for byte, and the resized nw x nh frame is never
 * written.  win i32 [B][4] = (nh, nw, top, left): the full resized size and the window's origin in it, computed by the caller as
 * torchvision does (the shorter side becomes `resize`, the other int(resize * other / shorter); nh = H_b, nw = W_b when the shorter
 * side already equals `resize`; top = round((nh - crop) / 2.0), half to even, likewise left).  The taps are built on the device in
 * Resample.c's double arithmetic for the full resized size, for the window's crop columns and rows only (one launch); the
 * horizontal pass runs over the source rows the window's vertical taps read, into a u8 temporary, then the vertical pass.
 *   workspace: 16-byte aligned (PM_EALIGN otherwise), at least pm_aug_resize_center_crop_workspace(B, Hmax, Wmax, resize, crop,
 *   &bytes) bytes (PM_EINVAL otherwise, as for a NULL pointer); it is sized for resized sides >= resize, which the rule above gives.
 *   PM_ESHAPE: B outside 1..65535, crop < 1, crop > resize (torchvision pads there), a non-positive size.  Every refusal returns
 *   before the first launch.  The tables are device memory and are trusted as those of pm_aug_resized_crop_ragged_u8 are: H_b <=
 *   Hmax, W_b <= Wmax, frame b inside src, the window inside nh x nw.  Reads stay inside frame b and writes inside dst and the
 *   queried workspace whatever win holds. */
int pm_aug_resize_center_crop_workspace(int B, int Hmax, int Wmax, int resize, int crop, size_t* bytes);
int pm_aug_resize_center_crop_ragged_u8(const unsigned char* src, const long long* offset, const int* hw, const int* win,
                                        unsigned char* dst, int B, int Hmax, int Wmax, int resize, int crop, void* workspace,
                                        size_t ws_bytes, void* stream);

/* ColorJitter: per sample, ops in `order` (0 brightness, 1 contrast, 2 saturation, 3 hue; -1 = none): ImageEnhance blends (float32,
 * truncating / clipping as Blend.c), contrast against int(mean luminance + 0.5) of the image as it stands before that op, hue as
 * an HSV round trip with H += hue_shift (uint8 wrap-around; hue_shift = uint8(hue_factor * 255)).  lsum: u64 [B] scratch.
 * Two launches (exact integer luminance sum, then the chain); src and dst may be the same buffer only if order has no contrast.
 * B <= 65535 (the sample is a grid dimension): a larger batch is refused with PM_ESHAPE before anything is enqueued. */
typedef struct pm_aug_jitter {
  int order[4];
  float brightness, contrast, saturation;
  int hue_shift;
} pm_aug_jitter;
int pm_aug_color_jitter_u8(const unsigned char* src, unsigned char* dst, const pm_aug_jitter* jitter, unsigned long long* lsum,
                           int B, int H, int W, void* stream);

/* GaussianBlur: separable ksize-tap convolution with reflect padding in f32 (taps f32 [B][ksize], one row per sample: the
 * caller evaluates torchvision's _get_gaussian_kernel1d for its sigma), taps summed in index order with separate multiply and
 * add, rint + clamp back to u8.  tmp f32 [B][H][W][3].  ksize odd, ksize / 2 < min(H, W).
 * Exactness: bit for bit against oracle/augment_ref.py (two separable f32 passes in this summation order).  torchvision 0.10's
 * tensor path builds the 2-D kernel (outer product of the 1-D taps) and runs ONE depthwise conv2d: different f32 rounding, so
 * after rint a few pixels can differ from the reference transform by 1 grey level (the oracle agrees with a float64 2-D
 * convolution to <= 1 level, > 99 % of pixels exactly); torchvision is absent here, so this stage is tolerance +-1 LSB, unpinned. */
int pm_aug_gaussian_blur_u8(const unsigned char* src, float* tmp, unsigned char* dst, const float* taps, int ksize, int B, int H,
                            int W, void* stream);

/* Flips, then rotation (Image.rotate(angle, NEAREST, expand=False, fillcolor=0)), then either the rotated u8 frame (to_f32 = 0,
 * dst u8 [B][H][W][3]) or ToTensor + Normalize (to_f32 = 1, dst f32 [B][3][H][W], as pm_preprocess_u8).  Per sample:
 * mode 0 = Pillow's 16.16 fixed-point inverse map, xin = (a2 + a0 x + a1 y) >> 16, yin = (a5 + a3 x + a4 y) >> 16 (coefficients
 * built by the caller as Image.rotate + affine_fixed do); 1 = no rotation; 2 / 3 / 4 = 180 / 90 / 270 degrees (Image.rotate's
 * transpose fast paths; 90 / 270 need H == W).  flips: bit 0 horizontal, bit 1 vertical, applied BEFORE the rotation. */
typedef struct pm_aug_geom {
  int mode, a0, a1, a2, a3, a4, a5, flips;
} pm_aug_geom;
int pm_aug_geometry_u8(const unsigned char* src, const pm_aug_geom* geom, void* dst, int to_f32, int B, int H, int W, float mean_r,
                       float mean_g, float mean_b, float std_r, float std_g, float std_b, void* stream);

/* Eval-time perturbations of PerRowPerturbations (classification/data/transforms.py:143-203; Exp-5A/5B feed them to the evaluation
 * forward path) on the resized uint8 frames, u8 [B][H][W][3]:
 *   "blur*": ImageFilter.GaussianBlur(radius=sigma) = Pillow's BoxBlur.c, `passes` extended-box passes per axis in UINT32 fixed
 *            point.  Per sample: radius = (int) r, ww = (UINT32)((float) 2^24 / (r * 2 + 1)), fw = (2^24 - (2 radius + 1) ww) / 2
 *            with r = _gaussian_blur_radius(sigma, passes) in float32 (built by the caller: data.py pil_box_blur_params);
 *            radius < 0: the sample passes through unchanged.  tmp: u8 [B][H][W][3] scratch; src may equal dst, tmp must not.
 *   "occ*":  ImageDraw.rectangle([x0, y0, x1, y1], fill=0), corners inclusive, clipped to the frame; x1 < x0: nothing.  In place.
 *            B <= 65535 (the sample is a grid dimension), else PM_ESHAPE.
 *   "bc*":   pm_aug_color_jitter_u8 with order {0, 1, -1, -1}.
 *   "jpeg*": img.save(format="JPEG", quality=q, optimize=False, subsampling=0) and back (transforms.py:78-85) WITHOUT a bitstream:
 *            entropy coding is lossless, so the round trip is libjpeg's integer pipeline -- RGB -> YCbCr (jccolor.c), 4:4:4, islow
 *            forward DCT (jfdctint.c), Annex-K tables scaled by q (jcparam.c, baseline), quantise / dequantise (jcdctmgr.c), islow
 *            inverse DCT (jidctint.c), YCbCr -> RGB (jdcolor.c); sides that are not multiples of 8 are edge-replicated and cropped.
 *            quality: int [B], 1..100; <= 0: the sample is copied.  src may equal dst.
 * Bit for bit against oracle/augment_ref.py, which is pinned by running the reference's own PerRowPerturbations (Pillow 12.2 with
 * its bundled libjpeg-turbo). */
typedef struct pm_aug_boxblur {
  int radius;
  unsigned int ww, fw;
} pm_aug_boxblur;
int pm_aug_pil_gaussian_blur_u8(const unsigned char* src, unsigned char* tmp, unsigned char* dst, const pm_aug_boxblur* prm,
                                int passes, int B, int H, int W, void* stream);
int pm_aug_occlude_u8(unsigned char* img, const int* rects, int B, int H, int W, void* stream);
int pm_aug_jpeg_roundtrip_u8(const unsigned char* src, unsigned char* dst, const int* quality, int B, int H, int W, void* stream);

/* Baseline JPEG decode of a batch of files -- what the reference's DataLoader workers do with Pillow (datasets.ImageFolder's
 * pil_loader: Image.open(f).convert("RGB"), mae/main_pretrain.py:161-190), bit for bit with its libjpeg-turbo, for 8-bit
 * Huffman-coded sequential files with one scan, grey or YCbCr 4:4:4 / 4:2:2 / 4:2:0, any restart interval.  The host
 * (ssl4polyp_amd/jpeg.py) parses and packs; here: entropy decode (jdhuff.c, one lane per restart interval) -> dequantise + islow
 * inverse DCT (jidctint.c) -> fancy upsampling (jdsample.c) + YCbCr -> RGB (jdcolor.c), packed HWC uint8 into `out`; frames the
 * host decoded itself (fallback) are copied to their slots.
 *   entropy: the unstuffed restart intervals, each on a 16-byte boundary, zero-padded; 16-byte aligned, entropy_bytes a multiple
 *     of 16.
 *   intervals int32 [n_intervals][8] = (frame, word offset, byte length, first MCU, MCU count, first subsequence, 0, 0); word 5
 *     is read by pm_jpeg_decode_parallel only.
 *   frames int32 [n_frames][32] = (H, W, components, luma h / v sampling, MCU columns / rows, restart interval, DC / AC /
 *     quantisation table per component, first coefficient block per component, output byte offset lo / hi, first pixel lo / hi).
 *   huff [n_huff][1024]: derived Huffman tables (jpeg.py derive_huffman); quant int32 [n_quant][64], natural order.
 *   fallback_table [n_fallback][3] = (offset in `fallback`, offset in `out`, bytes).
 *   Workspace: coef int16 [blocks * 64] and planes uint8 [blocks * 64], blocks = the batch's coefficient blocks; pixels = the
 *   device frames' pixels.  A table row that would address memory outside these sizes is skipped. */
int pm_jpeg_decode(const unsigned char* entropy, long entropy_bytes, const int* intervals, int n_intervals, const int* frames,
                   int n_frames, const unsigned char* huff, int n_huff, const int* quant, int n_quant, const unsigned char* fallback,
                   long fallback_bytes, const long long* fallback_table, int n_fallback, short* coef, unsigned char* planes,
                   long blocks, long pixels, unsigned char* out, long out_bytes, void* stream);

/* pm_jpeg_decode with the entropy stage parallel INSIDE a restart interval (files without restart markers are one interval): same
 * arguments, same bytes in `out`.  The host cuts every interval from its start into ceil(byte length / 128) subsequences numbered
 * through the interval rows in order: word 5 of an interval row is its first subsequence (the exclusive scan of the counts) and
 * subseq int32 [n_subseq] names the row of every subsequence.  One lane per subsequence decodes from a guessed state; the guesses
 * are corrected inside a 256-lane workgroup and, over `sync_rounds` (0..8) further launches, across workgroups; an interval is
 * accepted only if every lane's entry state equals its predecessor's exit state (which proves them the sequential decoder's
 * states); every other interval is decoded by one lane as in pm_jpeg_decode.  Nothing is read back and nothing waits on another
 * workgroup: 1 + sync_rounds + 3 launches replace the one of pm_jpeg_decode.
 *   workspace: 16-byte aligned, at least pm_jpeg_decode_workspace(n_intervals, n_subseq, &bytes) bytes; its contents on entry do
 *     not matter.  A smaller one is PM_EINVAL.
 *   stats (optional, device): int32 [5] = subsequences, intervals, intervals decoded sequentially, in-workgroup steps of the busiest
 *     workgroup, cross-workgroup rounds in which an entry changed. */
int pm_jpeg_decode_workspace(int n_intervals, int n_subseq, size_t* bytes);
int pm_jpeg_decode_parallel(const unsigned char* entropy, long entropy_bytes, const int* intervals, int n_intervals, const int* frames,
                            int n_frames, const unsigned char* huff, int n_huff, const int* quant, int n_quant,
                            const unsigned char* fallback, long fallback_bytes, const long long* fallback_table, int n_fallback,
                            short* coef, unsigned char* planes, long blocks, long pixels, unsigned char* out, long out_bytes,
                            const int* subseq, int n_subseq, int sync_rounds, void* workspace, size_t ws_bytes, int* stats,
                            void* stream);

/* The first two stages of pm_jpeg_decode_parallel alone: entropy decode + inverse DCT into the component planes (the same kernels,
 * the same arguments without the fallback frames and the output).  No RGB frame is written; pm_jpeg_resized_crop_u8 reads the
 * planes. */
int pm_jpeg_decode_planes(const unsigned char* entropy, long entropy_bytes, const int* intervals, int n_intervals, const int* frames,
                          int n_frames, const unsigned char* huff, int n_huff, const int* quant, int n_quant, short* coef,
                          unsigned char* planes, long blocks, const int* subseq, int n_subseq, int sync_rounds, void* workspace,
                          size_t ws_bytes, int* stats, void* stream);

/* pm_aug_resized_crop_ragged_u8 of a decoded JPEG batch without its packed RGB frames: box [B][4] = (top, left, h, w) inside frame b
 * of hw [B][2] -> dst [B][out][out][3].  The horizontal pass fetches every source pixel from the planes pm_jpeg_decode_planes left
 * (fancy chroma upsampling + YCbCr -> RGB per fetched pixel, the arithmetic of pm_jpeg_decode's last stage) or, for a frame the host
 * decoded, from its RGB bytes in `fallback`; the taps, the vertical pass and the workspace layout are those of
 * pm_aug_resized_crop_ragged_u8, so the bytes equal decoding to RGB first and cropping then.
 *   source int32 [B] (device): >= 0 the row of `frames` sample b is, -1 - k row k of fallback_table.
 *   planes / blocks / frames / fallback / fallback_table: as in pm_jpeg_decode.
 *   workspace: 16-byte aligned, at least pm_jpeg_resized_crop_workspace(B, Hmax, Wmax, out, &bytes) bytes (PM_EINVAL otherwise);
 *   B <= 65535.  The tables are trusted as those of pm_aug_resized_crop_ragged_u8 are (the caller validates boxes against hw); the
 *   horizontal pass additionally skips a sample whose tables do not fit together (a frame row outside `blocks`, a size that is not
 *   hw[b], a box outside the frame, fallback bytes outside the buffer), so nothing outside the buffers is read -- but the vertical
 *   pass still runs for it: dst[b] is then undefined (whatever the workspace held). */
int pm_jpeg_resized_crop_workspace(int B, int Hmax, int Wmax, int out, size_t* bytes);
int pm_jpeg_resized_crop_u8(const unsigned char* planes, long blocks, const int* frames, int n_frames, const unsigned char* fallback,
                            long fallback_bytes, const long long* fallback_table, int n_fallback, const int* source, const int* hw,
                            const int* box, unsigned char* dst, int bicubic, int B, int Hmax, int Wmax, int out, void* workspace,
                            size_t ws_bytes, void* stream);

/* One transformer block forward for one range of samples in ONE call (timm Block: models_mae.py:39-41,53-55,166-167,
 * 186-187; models.py:122-123,204-205):  x_mid = x + proj(attn(LN1 x));  x_out = x_mid + fc2(gelu(fc1(LN2 x_mid))).
 * Host-side composition of pm_layernorm_fwd / pm_gemm_ex / pm_attention_fwd on `stream`, launch for launch what a caller
 * would issue itself -- for hosts where ~27 separate calls per block cost more than the block takes to run.  Every
 * pointer addresses row 0 of the range (rows = samples * N tokens); buffers are the saved-for-backward activations:
 * ln1 / qkv [rows, 3D] / attn / ln2 / h_pre / h_act [rows, Hd] act-typed, x / x_mid / x_out f32 [rows, D], mean / rstd f32
 * [rows], lse f32 [samples * heads * N].  h_pre may be NULL when no backward will run through the block (evaluation, a frozen block
 * under a frozen front): fc1's GELU epilogue then stores the activation only.  The descriptor is plain data: build it once, keep it,
 * pass it every step. */
typedef struct pm_block_fwd_desc {
  const float* x;
  float* x_mid;
  float* x_out;
  void* ln1;
  float* mean1;
  float* rstd1;
  void* qkv;
  float* lse;
  void* attn;
  void* ln2;
  float* mean2;
  float* rstd2;
  void* h_pre;
  void* h_act;
  const float *norm1_w, *norm1_b, *norm2_w, *norm2_b;  /* f32 [D] */
  const void *qkv_w, *proj_w, *fc1_w, *fc2_w;          /* act-typed [out, in] as nn.Linear stores them */
  const float *qkv_b, *proj_b, *fc1_b, *fc2_b;         /* f32 */
  int rows, samples, N, D, Hd, heads;
  int dtype;        /* PM_BF16 / PM_F32: activation and matrix type */
  int gemm_variant; /* pm_gemm_opts.variant for the four GEMMs (0 = the dispatcher's heuristics) */
  float eps;
} pm_block_fwd_desc;
int pm_vit_block_fwd(const pm_block_fwd_desc* d, void* stream);

/* The backward of that block in ONE call (autograd of the timm Block through engine_pretrain.py:65 / tc.py:4533), for a
 * fully trainable block whose four weight gradients fit pm_wgrad_group:
 *   on `stream`:       [wait ev_join]  dfc2 (dGELU) -> dfc1 -> LN2' -> dproj -> attention' -> dqkv -> LN1'
 *   on `side_stream`:  after ev_fork (recorded behind attention'): pm_wgrad_group(fc2, fc1 + bias, proj, qkv + bias) -> ev_done
 * With two_groups != 0 (and an MLP pair that alone has >= 64 whole-K tiles; otherwise the flag is ignored) the weight
 * gradients go out as two launches on two side streams, each as soon as its operands exist:
 *   on `side_stream`:   after ev_fork  (recorded behind dfc2):       pm_wgrad_group(fc2, fc1 + bias)  -> ev_done
 *   on `side_stream2`:  after ev_fork2 (recorded behind attention'): pm_wgrad_group(proj, qkv + bias) -> ev_done2
 * so that the 72 + 36 workgroups of a ViT-B block are spread over the whole dgrad chain (the second launch runs on into the
 * next block's dfc2, which then shares the chip with 36 workgroups instead of 108); the block's matrix gradients are final
 * once BOTH events have fired.
 * dx / dx_act: gradient of the block output (f32 + act copy); dmid / dmid_act: residual gradient between the branches;
 * din / din_act: gradient of the block input (outputs).  Vector gradients are += targets; g_below_bias receives the column
 * sums of din (bias gradient of the Linear that produced the block input), NULL when there is none; accumulate bit j
 * (0 qkv, 1 proj, 2 fc1, 3 fc2): dW += instead of dW =.  ev_join (optional), ev_fork, ev_done are hipEvent_t of the caller:
 * ev_done fires when this block's matrix gradients are final and its operands may be overwritten.  The library creates,
 * keeps and frees nothing.  The weight-gradient group is validated (pm_wgrad_group_plan: shapes, alignment; and a k-sliced
 * group's ws_group_bytes against the plan's slab size -- too small is PM_EINVAL, not a silent fall-back to whole-K 256x128 tiles)
 * BEFORE the first launch: a refusal (PM_ESHAPE / PM_EALIGN / PM_EINVAL) returns with nothing enqueued on either stream, and
 * the caller falls back to per-kernel calls.  Any later non-zero status is a launch failure (PM_ELAUNCH). */
typedef struct pm_block_bwd_desc {
  const float* x_in;
  const float* x_mid;
  const void *ln1, *qkv, *attn, *ln2, *h_pre, *h_act;
  const float *mean1, *rstd1, *mean2, *rstd2, *lse;
  const float *norm1_w, *norm2_w;
  const void *qkv_w, *proj_w, *fc1_w, *fc2_w;
  const float* dx;
  const void* dx_act;
  float* dmid;
  void* dmid_act;
  float* din;
  void* din_act;
  void *d_hidden, *d_qkv, *d_ln, *d_attn;
  float* delta;
  float *g_norm1_w, *g_norm1_b, *g_norm2_w, *g_norm2_b;
  float *g_qkv_w, *g_proj_w, *g_fc1_w, *g_fc2_w;
  float *g_qkv_b, *g_proj_b, *g_fc1_b, *g_below_bias;
  void* ws_ln;
  size_t ws_ln_bytes;
  void* ws_group;
  size_t ws_group_bytes;
  void *side_stream, *ev_join, *ev_fork, *ev_done;
  int samples, N, D, Hd, heads, dtype, gemm_variant, group_blocks, accumulate;
  int two_groups;                                /* see above; needs the three handles below */
  void *side_stream2, *ev_fork2, *ev_done2;
} pm_block_bwd_desc;
int pm_vit_block_bwd(const pm_block_bwd_desc* d, void* stream);

/* Top of the fine-tune forward (models.py:127,134-139 / 209,216-221): final LayerNorm, token selection, lin_head.
 *   pool = 0 (out_token "cls"):     feat[b] = LN(x[b, 0])                 (only row 0 is normalised)
 *   pool = 1 (out_token "spatial"): feat[b] = mean_{n >= 1} LN(x[b, n])   (x[:, 1:].mean(1))
 *   logits = feat W^T + bias when W != NULL (head=True); W == NULL returns the features only (head=False).
 * x f32 [B, N, D]; feat f32 [B, D]; mean / rstd f32 [B] (pool 0) or [B, N] (pool 1, row 0 unused); xhat_mean f32 [B, D]
 * (pool 1 only: the pooled normalised rows, saved for backward); logits f32 [B, n_class].  D <= 1024. */
int pm_vit_head_fwd(const float* x, int N, int pool, const float* gamma, const float* beta, const float* W,
                    const float* bias, float* feat, float* xhat_mean, float* mean, float* rstd, float* logits, int B, int D,
                    int n_class, float eps, void* stream);
/* Backward.  Gradient source: dlogits f32 [B, n_class] (with W), or dfeat f32 [B, D] (head=False; then dlogits / W / dW /
 * dbias are unused).  dx f32 [B,N,D] is fully written (rows that do not reach the feature get zeros) together with its
 * act-typed copy dx_act (optional); dx == NULL = frozen backbone, nothing below is needed.  dW / dbias / dgamma / dbeta
 * (+=, each optional) are summed over the batch in a fixed order. */
int pm_vit_head_bwd(const float* dlogits, const float* dfeat, const float* x, int N, int pool, const float* gamma,
                    const float* W, const float* feat, const float* xhat_mean, const float* mean, const float* rstd,
                    float* dx, void* dx_act, int act_dtype, float* dW, float* dbias, float* dgamma, float* dbeta, int B,
                    int D, int n_class, void* stream);
/* The same with pool = 0 and a head (the shipped configuration: utils/__init__.py:29,52 default out_token "cls"). */
int pm_cls_head_fwd(const float* x, int N, const float* gamma, const float* beta, const float* W, const float* bias,
                    float* xn, float* mean, float* rstd, float* logits, int B, int D, int n_class, float eps,
                    void* stream);
int pm_cls_head_bwd(const float* dlogits, const float* x, int N, const float* gamma, const float* W, const float* xn,
                    const float* mean, const float* rstd, float* dx, void* dx_act, int act_dtype, float* dW,
                    float* dbias, float* dgamma, float* dbeta, int B, int D, int n_class, void* stream);

/* Supervised loss of the fine-tune loop on the logits (train_classification.py:3347-3374 _compute_supervised_loss,
 * 6086-6104 loss construction), value and gradient in one launch:
 *   n_class == 2 ("binary_bce"): z = l[:,1] - l[:,0]; BCEWithLogitsLoss(pos_weight)(z, y), mean over the batch;
 *                                pos_weight: f32 DEVICE scalar or NULL (= 1)
 *   n_class  > 2: CrossEntropyLoss(weight = class_weights f32 [n_class] or NULL), weighted mean.
 * targets int64 [B]; loss f32 [1]; dlogits f32 [B, n_class] = d loss / d logits.  One block, fixed summation order. */
int pm_supervised_loss_fwd(const float* logits, const long long* targets, const float* pos_weight,
                           const float* class_weights, float* loss, float* dlogits, int B, int n_class, void* stream);
/* out[i] = x[i] * scale[0] (scale: f32 device scalar) -- chains an upstream d loss into the saved dlogits. */
int pm_scale(const float* x, const float* scale, float* out, long n, void* stream);

/* out[i] = dy[i] * gelu_erf'(pre[i]) over n elements of `dtype` (n % 4 == 0): the backward of timm Mlp's nn.GELU
 * (models_mae.py:39-41 through timm Block) as a stand-alone pass, for callers that compose blocks from the per-kernel ops
 * (the training step gets the same product from the dfc2 GEMM's PM_EPI_DGELU epilogue).  out may alias dy. */
int pm_dgelu(const void* dy, const void* pre, void* out, int dtype, long n, void* stream);

/* Fused multi-tensor AdamW over one flat f32 parameter range (torch.optim.AdamW semantics,
 * tc.py:5766-5768 / main_pretrain.py:218) that also refreshes the act-typed shadow copy used by the GEMMs.
 * grad_scale multiplies the gradient (1/world, 1/accum).  step >= 1.  p, g, m, v and an f32 shadow are moved as 16-byte
 * vectors, a 16-bit shadow as 8-byte ones: a pointer not so aligned is PM_EALIGN before any launch (pm_adamw_dev and the
 * segments of pm_adamw_segments / _list likewise). */
int pm_adamw(float* p, const float* g, float* m, float* v, void* shadow, int shadow_dtype, long n, float lr,
             float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale, void* stream);

/* hipGraph-replayable form of the same update: the hyper-parameters live in DEVICE memory, one 16-float record per
 * param group: [0] lr [1] beta1 [2] beta2 [3] eps [4] weight_decay [5] grad_scale [6] step [7] bc1 [8] 1/sqrt(bc2)
 * [9] skip flag [10] 1 / loss scale (both written by pm_loss_scale_update; 0 = no loss scaling).
 * pm_adamw_tick advances step and the bias corrections of `n_groups` records; pm_adamw_dev applies one record to a
 * flat range (gradient x [5] x [10]); both return without touching anything while [9] is set.  A captured step therefore
 * replays correctly while the host changes lr between replays. */
int pm_adamw_tick(float* hyper, int n_groups, void* stream);
int pm_adamw_dev(float* p, const float* g, float* m, float* v, void* shadow, int shadow_dtype, long n,
                 const float* hyper, void* stream);

/* The whole update of a step as ONE call, for an update that runs on a side stream beside the next forward:
 *   [wait for `wait_event` ->] pm_adamw_tick(hyper, n_groups) -> per segment: the pm_adamw_dev update [-> record done_event]
 * all on `stream`.  A segment is one pm_adamw_dev argument list (its `hyper` points at the record of its group inside the
 * `hyper` array) plus an optional hipEvent_t of the caller that is recorded behind its launch, so that a consumer on another
 * stream can wait for exactly the ranges it reads.  max_blocks bounds the workgroups of every launch (pm_adamw_grid): 0 = the
 * full grid of pm_adamw_dev.  The results do not depend on it: every element is updated by the same expression whatever the
 * grid.  Every argument is checked before the first enqueue (PM_EINVAL: a NULL pointer or an unknown shadow dtype; PM_ESHAPE:
 * no segments, n <= 0, n % 4 != 0, max_blocks < 0), so a refusal leaves the stream untouched. */
typedef struct pm_adamw_segment {
  float* p;
  const float* g;
  float *m, *v;
  void* shadow;        /* optional act-typed copy of p, refreshed by the same launch */
  int shadow_dtype;
  long n;
  const float* hyper;  /* this segment's 16-float record */
  void* done_event;    /* optional hipEvent_t */
} pm_adamw_segment;
int pm_adamw_segments(const pm_adamw_segment* segs, int n_segs, float* hyper, int n_groups, void* wait_event, void* stream,
                      int max_blocks);
/* Workgroups one update launch over n elements uses under the bound max_blocks (host arithmetic only; PM_ESHAPE for n <= 0,
 * n % 4 != 0 or max_blocks < 0). */
int pm_adamw_grid(long n, int max_blocks);

/* Dynamic loss scaling of precision mode fp16, on the device: GradScaler.step() + update() of the reference's AMP loop
 * (train_classification.py:4533-4546; engine_pretrain.py:65-72 via mae/util/misc.py:252-282) without the host read-back.
 * state: f32[8] = [0] scale [1] growth tracker [2] found_inf of the last step [3] skipped steps [4] steps [5] 1/scale used.
 * stats: the pm_grad_stats triple of THIS step's (scaled) gradients.  Writes the skip flag and 1/scale into the `n_groups`
 * AdamW records, then moves the scale: x backoff_factor after a non-finite step, x growth_factor after growth_interval
 * clean steps in a row (a grown scale that overflows f32 is not taken: the scale stays, as in torch).  Launch order on one stream: pm_grad_stats ..., pm_loss_scale_update, pm_adamw_tick, pm_adamw_dev ... */
int pm_loss_scale_update(float* state, const float* stats, float* hyper, int n_groups, float growth_factor,
                         float backoff_factor, int growth_interval, void* stream);

/* One-pass gradient statistics over a flat f32 range: out[0] += sum(g^2), out[1] += #NaN, out[2] += #Inf
 * (the device-side counterpart of tc.py:1437-1454 _compute_grad_norm and misc.py:387-400 detect_grad_anomalies). */
int pm_grad_stats(const float* g, long n, float* out, void* stream);

/* Per-group gradient norms and clipping by global norm, deterministic (no float atomics): the reference's per-group norms after
 * scaler.unscale_ (train_classification.py:4534-4544, _compute_grad_norm :1437-1454) and its clip_grad_norm_ between unscale_ and
 * step (mae/util/misc.py:268-279), without touching the update kernels: the clip coefficient goes into slot [10] of the AdamW
 * records, the factor pm_adamw_dev already multiplies every gradient by ([10] = 1 / loss scale x clip coefficient; 0 = neither).
 *
 * pm_grad_norms: one pass over `n_segs` flat f32 gradient ranges (n % 4 == 0, 16-byte aligned; padding holds zeros), each
 * belonging to one of `n_groups` groups.  Every value is squared and accumulated in f64 by a fixed map and fixed trees; the grid
 * depends on the segment sizes only, so the bits do not depend on stream, overlap or capture.  Writes
 *   sumsq f64 [n_groups]  sum(g^2) per group (0 for a group without a segment)
 *   stats f32 [3]         [sum(g^2), #NaN, #Inf] over everything, pm_grad_stats' layout (overwritten, not accumulated): what
 *                         pm_loss_scale_update reads, so this pass REPLACES the pm_grad_stats pass of a loss-scaled step.
 * workspace: caller-owned, 8-byte aligned, at least pm_grad_norms_workspace(n_segs, n_groups) bytes; fully rewritten.
 *
 * pm_grad_clip: one small launch.  With s_g = record_g[5] x (scaled && record_g[10] != 0 ? record_g[10] : 1) -- `scaled` says
 * that pm_loss_scale_update wrote [10] THIS step; without it [10] counts as 1 whatever an earlier clip left there --
 *   total = sqrt(sum_g sumsq[g] s_g^2),  coef = min(1, max_norm / (total + 1e-6))   (torch.nn.utils.clip_grad_norm_, in f64)
 * and, when `clip` is set, record_g[10] = (scaled && [10] != 0 ? [10] : 1) x coef for every group (one f32 rounding; coef and the
 * product are held to >= FLT_MIN so that [10] never becomes the 0 that means "no scaling").  A non-finite total gives a
 * non-finite coef, as torch does: under loss scaling the skip flag [9] is set then and the update touches nothing; without a
 * scaler the update applies NaN, exactly like clip_grad_norm_ + step.  clip == 0: norms only, coef = 1, `hyper` is left alone.
 *   record f64 [n_groups + 3]  sqrt(sumsq[g]) s_g per group, total, coef, max_norm (+inf when clip == 0)
 * Launch order on one stream:
 *   pm_grad_norms, [pm_loss_scale_update(stats),] pm_grad_clip, pm_adamw_tick, pm_adamw_dev ... (or pm_adamw_segments)
 * Refusals return before any stream call: PM_EINVAL (a NULL pointer, a group index outside [0, n_groups), a short workspace,
 * clip with max_norm <= 0 or NaN), PM_ESHAPE (no segments or groups, n <= 0, n % 4 != 0), PM_EALIGN. */
typedef struct pm_grad_segment {
  const float* g;
  long n;
  int group;
} pm_grad_segment;
int pm_grad_norms_workspace(int n_segs, int n_groups, size_t* bytes);
int pm_grad_norms(const pm_grad_segment* segs, int n_segs, int n_groups, void* workspace, size_t ws_bytes, double* sumsq,
                  float* stats, void* stream);
int pm_grad_clip(const double* sumsq, float* hyper, int n_groups, double max_norm, int clip, int scaled, double* record,
                 void* stream);

/* Per-parameter steps (torch.optim.AdamW keeps state[p]["step"] per parameter; a parameter that first receives a gradient at
 * optimizer step T starts its bias corrections at 1): a param group may own SEVERAL of the 16-float records above, one per
 * "cohort" of its parameters that share a step history.  The caller writes the group's [0..5] into each of them; [6..8] are the
 * cohort's own; pm_loss_scale_update takes the record count as its n_groups.  The update kernels are the same: a segment points
 * at its cohort's record.  Two int lists describe the plan, each given twice: the device copy the kernel reads (fixed address,
 * so a captured step replays it) and the caller's host copy of the same entries, which is what is checked before any enqueue.
 *
 * pm_adamw_tick_list: pm_adamw_tick (same skip rule, same f64 arithmetic, so a cohort at step t holds the bits a group at step t
 *   holds) for the `n_list` records `list` names, out of `n_records`.  PM_EINVAL: a NULL pointer, an entry outside [0, n_records),
 *   entries not strictly ascending; PM_ESHAPE: n_list <= 0 or > n_records.
 * pm_adamw_segments_list: pm_adamw_segments with that tick in place of the tick over every record; every segment's `hyper` must
 *   point at one of the n_records records (PM_EINVAL).  Checks, wait event, done events and max_blocks as pm_adamw_segments.
 * pm_grad_clip_cohorts: pm_grad_clip where sumsq holds one sum per RECORD (pm_grad_norms with the segments tagged by record and
 *   n_groups = n_records) and group_of[r] names record r's group.  A group's sum is the sum of its records' in ascending record
 *   order, in f64; then pm_grad_clip's arithmetic, s_g read from the group's first record; the new [10] goes into all n_records
 *   records; `record` is the same f64 [n_groups + 3].  With n_records == n_groups and group_of[r] == r the bits are pm_grad_clip's.
 *   PM_EINVAL also for an entry of group_of outside [0, n_groups). */
int pm_adamw_tick_list(float* hyper, int n_records, const int* list, const int* list_host, int n_list, void* stream);
int pm_adamw_segments_list(const pm_adamw_segment* segs, int n_segs, float* hyper, int n_records, const int* list,
                           const int* list_host, int n_list, void* wait_event, void* stream, int max_blocks);
int pm_grad_clip_cohorts(const double* sumsq, float* hyper, int n_records, const int* group_of, const int* group_of_host,
                         int n_groups, double max_norm, int clip, int scaled, double* record, void* stream);

/* Scratch sizes.  Every workspace is caller-owned; these return the byte count that enables the deterministic
 * (two-stage, fixed-order) form of the op for the given shape, 0 when the op needs none.
 *   pm_gemm_workspace_bytes: the split-K slabs pm_gemm_ws / pm_gemm_ex would use for this GEMM under `opts`.
 *   pm_workspace_bytes(kind, M, N): PM_WS_LAYERNORM_BWD (M rows, N = D), PM_WS_COLSUM (M x N matrix),
 *   PM_WS_UNSHUFFLE_BWD (N = D). */
enum pm_ws_kind { PM_WS_LAYERNORM_BWD = 1, PM_WS_COLSUM = 2, PM_WS_UNSHUFFLE_BWD = 4 };
size_t pm_gemm_workspace_bytes(int a_kmajor, int b_kmajor, int in_dtype, int M, int N, int K, const pm_gemm_opts* opts);
size_t pm_workspace_bytes(int kind, int M, int N);

/* ---- gradient exchange for hosts without torch.distributed (SURVEY 8-b `pm_comm_*`) --------------------------------------
 * A handle over RCCL (bound at run time: PM_EARCH when no librccl can be loaded).  Replaces DistributedDataParallel's reducer of
 * the reference (mae/main_pretrain.py:212-214, train_classification.py:5746-5750) for a C / C++ host; the Python host does the
 * same through torch.distributed (parallel.GradSync).  One process per GPU: rank 0 calls pm_comm_unique_id and hands the 128
 * bytes to the other ranks out of band (file, socket, environment); every rank then calls pm_comm_create on ITS device.
 * pm_comm_allreduce_f32 sums, in place, n_buckets slices base[lo[i] .. hi[i]) (element offsets) of one f32 range over all ranks
 * in one RCCL group on `stream` -- the flat gradient range needs no packing, a bucket is a slice; the caller orders `stream`
 * against its compute stream with events and divides by the world size where it consumes the sums (pm_adamw_dev grad_scale).
 * The handle is the one object this library creates; pm_comm_destroy frees it. */
typedef struct pm_comm pm_comm;
int pm_comm_unique_id(void* id128);
int pm_comm_create(pm_comm** out, const void* id128, int rank, int world);
int pm_comm_world(const pm_comm* c, int* rank, int* world);
int pm_comm_allreduce_f32(pm_comm* c, float* base, const long* lo, const long* hi, int n_buckets, void* stream);
int pm_comm_destroy(pm_comm* c);

/* ---- cluster-bootstrap replicates of the binary test metrics --------------------------------------------------------------
 * Replaces the loop of the reference's report modules (classification/analysis/exp*_report.py) over
 * common_metrics.sample_cluster_ids + compute_binary_metrics (common_metrics.py:100-232; eight scikit-learn calls on a gathered
 * sample per replicate).  A replicate is a multiset of the N scored frames: frame i counts w = (number of entries of draws[r]
 * that name cluster[i]) times.  M runs that scored the same frames share the draws (the paired comparisons of the reports).
 *   score   f64 [M, N]  probabilities of the positive class, finite
 *   order   i32 [M, N]  per run, the frame indices in descending score order (ties in any order)
 *   label   u8  [N]     0 / 1
 *   cluster i32 [N]     values in [0, C)
 *   draws   i32 [R, K]  cluster indices; -1 is padding
 *   tau     f64 [M]     decision threshold per run (prediction = score >= tau)
 *   out     f64 [R, M, 16] in the reference's key order: count, n_pos, n_neg, prevalence, tp, fp, tn, fn, auprc, auroc, recall,
 *           precision, f1, balanced_accuracy, mcc, loss.  Counts are exact; average precision and AUROC treat tied scores as one
 *           threshold, as sklearn's curves do; the f64 sums run in a fixed order, so equal inputs give equal bits however R is cut
 *           into calls.  A replicate without positives or without negatives gets what scikit-learn 1.7 returns for such a sample
 *           (AUROC NaN, average precision 0 without positives, empty ratios 0); an empty replicate is NaN beyond the counts.
 * Limits (PM_ESHAPE before any launch): 1 <= N, K, C <= 2^20, M <= 256, R <= 4096 per call, N * K < 2^31 (a replicate's total
 * weight fits 31 bits).  Table entries outside their range (an order index, a cluster, a draw) count as weight zero / no draw.
 * workspace: 16-byte aligned, at least pm_boot_metrics_workspace(N, M, R, K, C, &bytes) bytes (PM_EINVAL otherwise).  Its head
 * holds the sorted view of the runs (score, per-frame loss, cluster and label in `order`), which does not depend on the replicates.
 * sorted_ready = 0: the contents on entry do not matter and the view is built (one memset and three launches on `stream`).
 * sorted_ready != 0: the caller states that an earlier call on this stream with sorted_ready = 0 and the same score, order, label,
 * cluster, N, M and C built the view in this workspace (R may differ: the view lies before everything sized by R) and that nothing
 * else wrote there since; the view is reused (one memset and two launches).  This is how R replicates are cut into several calls. */
int pm_boot_metrics_workspace(int N, int M, int R, int K, int C, size_t* bytes);
int pm_boot_metrics(const double* score, const int* order, const unsigned char* label, const int* cluster, const int* draws,
                    const double* tau, double* out, int N, int M, int R, int K, int C, int sorted_ready, void* workspace,
                    size_t ws_bytes, void* stream);

/* ---- the same replicates per group of frames: perturbation tags, morphology strata ------------------------------------------
 * Replaces one pm_boot_metrics call per group on a gathered subset (the reference's per-tag metrics, train_classification.py:5256-5483,
 * and morphology strata, :3041-3089, exp3_report.compute_strata_metrics).  A group is a set of frames; groups may overlap (every
 * stratum holds every negative).  The memberships are expanded into E entries, one per (group, frame) pair, laid out as G segments:
 *   score   f64 [M, N]  as pm_boot_metrics takes it
 *   member  i32 [M, E]  per run, the frame index of every entry: segment g = entries seg[g] .. seg[g + 1] - 1 holds the frames of
 *                       group g in descending score order (ties in any order; the bits below hold for the order stated there).
 *                       An entry outside [0, N) (-1 = padding) has weight zero
 *   seg     i32 [G + 1] segment offsets, ON THE DEVICE, non-decreasing from 0 to at most E.  Values are clamped to [0, E] and a
 *                       segment whose start >= its end is empty, so no table can send an access outside the buffers
 *   label, cluster, draws, tau  as pm_boot_metrics takes them (clusters and draws are those of the whole set: a group's replicate
 *                       is the replicate of the set restricted to the group)
 *   out     f64 [R, M, G, 16] in pm_boot_metrics' key order.  One workgroup per (replicate, run, group) scans its own segment only:
 *           the work is proportional to E, not to G * N.  A tie group ends at the segment's end whatever score the next segment
 *           starts with, and scan tiles are laid from the segment's start, so group g's 16 values are, bit for bit, what
 *           pm_boot_metrics returns for the frames of g alone (gathered in the order of their entries' score ties) with the same
 *           cluster and draws -- and a group that lists every frame gives pm_boot_metrics' own bits.  An empty group, or one no
 *           frame of which was drawn, gives the empty replicate's row (counts 0, the rest NaN).
 * Limits (PM_ESHAPE before any launch): 1 <= N, K, C <= 2^20, 1 <= E <= 2^22, 1 <= G <= 2^16, M <= 256, R <= 4096 per call,
 * E * K < 2^31 (a segment's total weight fits 31 bits), R * M * G < 2^31 (one launch).
 * workspace: 16-byte aligned, at least pm_group_metrics_workspace(N, M, E, G, R, K, C, &bytes) bytes (PM_EINVAL otherwise, as for
 * a missing buffer; PM_EALIGN for a misaligned one).  Its head holds the prepared view of the entries [M, E] (score, per-frame
 * loss, cluster << 1 | label), then the counters mult [R, C].  sorted_ready as for pm_boot_metrics: 0 builds the view (one memset
 * and three launches on `stream`), != 0 states that an earlier call with the same score, member, label, cluster, N, M, E and C
 * built it here and reuses it (one memset and two launches).  The launcher reads no device data and does not synchronise. */
int pm_group_metrics_workspace(int N, int M, int E, int G, int R, int K, int C, size_t* bytes);
int pm_group_metrics(const double* score, const int* member, const int* seg, const unsigned char* label, const int* cluster,
                     const int* draws, const double* tau, double* out, int N, int M, int E, int G, int R, int K, int C,
                     int sorted_ready, void* workspace, size_t ws_bytes, void* stream);

/* ---- the decision threshold of a run, chosen on its validation scores ------------------------------------------------------
 * Replaces the reference's classification/metrics/thresholds.py: compute_policy_threshold (:299-390) for policy 0 f1_opt_on_val,
 * 1 youden_on_val, 2 val_opt_youden (the same objective as 1), and compute_youden_j_threshold (:68-110: scikit-learn's roc_curve
 * with drop_intermediate, first maximum of tpr - fpr, nextafter(max score, 1.0) when the curve's +inf point wins) for 3 youden.
 *   score        f64 [M, N]  probabilities of the positive class in [0, 1] (anything else, NaN included, is outside the contract:
 *                            no access leaves the buffers, the values are unspecified)
 *   order        i32 [M, N]  per run, the frame indices in descending score order, as pm_boot_metrics takes it; an entry outside
 *                            [0, N) is no frame (it belongs at the end of a run: it is placed at score 0 and counts for no class)
 *   label        u8  [N]     0 / 1
 *   previous_tau f64 [M]     the threshold carried into a run whose labels hold one class only; NaN = none (then 0.5)
 *   out          f64 [M, 16] tau, n_candidates, degenerate, objective, tp, fp, tn, fn, recall, precision, f1, tpr, fpr, youden_j,
 *                            n_unique, index.  Policies 0-2: n_unique is the number U of unique values of {0} + scores + {1}, the
 *                            candidates are all of them (U <= 200) or those at numpy.linspace(0, U - 1, 200, dtype=int), index is the
 *                            chosen candidate's.  Policy 3: n_candidates is the number of points roc_curve returns, n_unique the
 *                            number of distinct scores, index the chosen point's in the curve before points are dropped (0 = +inf).
 *                            One class only: degenerate = 1, n_candidates = 0, objective and n_unique NaN, tau = previous_tau if
 *                            finite (index = -2) else 0.5 (index = -1) with the counts taken there; policy 3 has no answer (tau NaN,
 *                            counts 0, index = -1).
 *   candidates   f64 [M, 200] or NULL: the candidate list of policies 0-2 in ascending order (one class only: tau alone), NaN beyond
 *                            it; all NaN for policy 3.
 * Counts are exact and every ratio is one f64 division of them, so the values are the reference's bit for bit.  One launch of one
 * workgroup per run on `stream`; nothing is read back, nothing is allocated.  Limits (PM_ESHAPE): 1 <= N <= 2^20, 1 <= M <= 256.
 * workspace: 16-byte aligned, at least pm_select_tau_workspace(N, M, &bytes) bytes (PM_EINVAL otherwise, as for a missing buffer or
 * a policy outside 0-3); its contents on entry do not matter. */
int pm_select_tau_workspace(int N, int M, size_t* bytes);
int pm_select_tau(const double* score, const int* order, const unsigned char* label, const double* previous_tau, int policy,
                  double* out, double* candidates, int N, int M, void* workspace, size_t ws_bytes, void* stream);

/* ---- linear probing of a frozen encoder (mae/main_linprobe.py) -------------------------------------------------------------
 * The launches the probe protocol adds beside the forward-only encoder: the global_pool feature, the BatchNorm1d + Linear head,
 * softmax cross-entropy with the accuracy counts of engine_finetune.evaluate, the head's weight gradients, and LARS
 * (mae/util/lars.py).  f32 throughout, fixed summation order (no float atomics), nothing allocated, the stream passed in; every
 * refusal (PM_EINVAL: a NULL pointer, a short workspace, eps < 0; PM_ESHAPE; PM_EALIGN) returns before the first launch.
 *
 * pm_pool_norm_fwd: feat[b] = LayerNorm_{gamma, beta, eps}(mean_{n >= 1} x[b, n, :]) -- models_vit.py:46-48 (global_pool), forward
 *   only (the encoder and fc_norm are frozen).  x f32 [B, N, D] (the last block's output, no final norm), feat f32 [B, D];
 *   N >= 2, D % 4 == 0, D <= 2048; everything 16-byte aligned.  x is read once.  workspace: pm_pool_norm_workspace bytes.
 *
 * pm_probe_head_fwd: BatchNorm1d(affine=False) over feat [B, D], then logits = xhat W^T + bias, W [C, D].  xhat [B, D] is saved.
 *   training != 0: batch mean and biased variance; running = (1 - momentum) running + momentum new, the running variance from the
 *     unbiased estimate (divisor B - 1), *num_batches_tracked += 1 (int64 on the device), as torch.nn.BatchNorm1d.  B < 2 is
 *     PM_ESHAPE (torch raises there too).
 *   training == 0: the same map through running_mean / running_var; nothing is updated (num_batches_tracked may be NULL).
 *   D % 4 == 0; W and xhat 16-byte aligned; B <= 65535.
 *
 * pm_probe_ce: torch.nn.CrossEntropyLoss() (mean over the batch) of logits [B, C] against int64 targets in [0, C), any C >= 1.
 *   loss f32 [1]; dlogits [B, C] = (softmax - onehot) / B x scale[0] (scale: a device scalar, 1 / accum_iter in training; dlogits
 *   NULL: not computed, scale may be NULL); correct int64 [2], overwritten: the rows whose target is correct at 1 and at
 *   k = min(5, C), a row being correct at k when fewer than k classes have a logit strictly greater than the target's.  A target
 *   outside [0, C) makes the loss NaN, counts as wrong and gets a zero gradient row.  workspace: pm_probe_ce_workspace bytes.
 *
 * pm_probe_head_bwd: dW [C, D] += dlogits^T xhat, dbias [C] += sum_b dlogits: one addition into what they held (gradient
 *   accumulation over accum_iter micro-batches).  There is no gradient with respect to the features.  C <= 65535.
 *
 * pm_lars_step: mae/util/lars.py:22-47 over n_segs tensors of ONE param group.  hyper: device f32 [4] = lr, weight decay,
 *   momentum, trust coefficient (read by the kernels, so a captured step follows an lr written between replays).
 *     is_matrix (p.ndim > 1): dp = g + wd p; q = tc |p| / |dp| if |p| > 0 and |dp| > 0, else 1; dp *= q
 *     otherwise:              dp = g                                 (no decay, no trust ratio)
 *     mu = momentum mu + dp;  p -= lr mu
 *   The norms are f64 sums of the squared f32 values over a fixed two-stage map that depends on the segment's length alone: a
 *   table of several segments gives the bits of one call per segment.  Any n >= 1, 4-byte alignment.
 *   workspace: 8-byte aligned, pm_lars_workspace(n_segs) bytes. */
typedef struct pm_lars_segment {
  float* p;
  const float* g;
  float* mu;
  long n;
  int is_matrix;
} pm_lars_segment;
int pm_pool_norm_workspace(int B, int N, int D, size_t* bytes);
int pm_pool_norm_fwd(const float* x, int B, int N, int D, const float* gamma, const float* beta, float eps, float* feat,
                     void* workspace, size_t ws_bytes, void* stream);
int pm_probe_head_fwd(const float* feat, int B, int D, int C, const float* W, const float* bias, float* running_mean,
                      float* running_var, long long* num_batches_tracked, int training, float momentum, float eps, float* xhat,
                      float* logits, void* stream);
int pm_probe_ce_workspace(int B, size_t* bytes);
int pm_probe_ce(const float* logits, const long long* target, int B, int C, const float* scale, float* loss, float* dlogits,
                long long* correct, void* workspace, size_t ws_bytes, void* stream);
int pm_probe_head_bwd(const float* dlogits, const float* xhat, int B, int D, int C, float* dW, float* dbias, void* stream);
int pm_lars_workspace(int n_segs, size_t* bytes);
int pm_lars_step(const pm_lars_segment* segs, int n_segs, const float* hyper, void* workspace, size_t ws_bytes, void* stream);

/* ---- end-to-end fine-tuning of the MAE encoder (mae/main_finetune.py, engine_finetune.py) ----------------------------------
 * What the recipe puts around the block stack: timm's Mixup / CutMix of the batch (mode "batch"), SoftTargetCrossEntropy over the
 * mixed, smoothed targets, the trainable global_pool (models_vit.py:46-48) and the plain Linear head.  Conventions of the probe
 * section: f32 throughout, fixed summation order (no float atomics), nothing allocated, the stream passed in; every refusal returns
 * before the first launch; everything 16-byte aligned unless stated.
 *
 * pm_mix_record: the draw of one step, on the DEVICE (the host writes it through pinned memory with an asynchronous copy, so no
 *   launch argument changes from step to step and a captured step follows new draws).  lam and one_minus_lam are both rounded from
 *   the host's doubles (one_minus_lam is NOT 1.f - lam).  use_cutmix != 0: the box rows [yl, yh) x columns [xl, xh).
 *
 * pm_mix_batch: x f32 [B, C, H, W] in place; sample b is paired with B - 1 - b (timm's x.flip(0)); one thread owns the same
 *   elements of both members of a pair.  B odd is PM_ESHAPE (timm asserts an even batch); C H W < 2^31.
 *     Mixup:   x_b <- fl(fl(lam x_b) + fl(one_minus_lam x_p)) and the same for the partner, from the OLD values; two products and
 *              one sum, never a fused multiply-add: torch's x.flip(0).mul_(1 - lam); x.mul_(lam).add_(.) bit for bit.
 *     CutMix:  inside the box the pair swaps its old values; outside nothing is read or written.  An empty box writes nothing; the
 *              box is clipped to the image; xl may have any alignment.
 *   enabled == 0: the host drew lam == 1 without a box -- every check, no launch.  (A record that holds that draw makes the
 *   launched kernel write nothing either.)  rec: 4-byte aligned.
 *
 * pm_soft_ce: timm's SoftTargetCrossEntropy over mixup_target, the targets never materialised.  logits [B, C], int64 target [B];
 *     off = smoothing / C, on = 1 - smoothing + off (in double, rounded to f32, as timm's one_hot stores them)
 *     t_b  = lam onehot(y_b; on, off) + one_minus_lam onehot(y_{B-1-b}; on, off)     (the two weights ADD when the classes coincide)
 *     loss = mean_b sum_c t_bc (lse_b - z_bc);   dlogits = (softmax - t) / B x scale[0]
 *   rec NULL: lam = 1, one_minus_lam = 0 -- then it is LabelSmoothingCrossEntropy(smoothing), and with smoothing = 0
 *   torch.nn.CrossEntropyLoss().  scale: a device scalar (1 / accum_iter), as for pm_probe_ce; dlogits NULL: not computed.  A target
 *   of the row or of its partner outside [0, C) makes the loss NaN and gives the row a zero gradient.  Any C >= 1, any B <= 65535
 *   (the middle row of an odd batch is its own partner).  4-byte alignment (target: 8).  workspace: pm_soft_ce_workspace bytes.
 *
 * pm_pool_norm_fwd_train: pm_pool_norm_fwd (same two-stage sum: feat has its bits) that also writes the pooled row [B, D] and
 *   mean / rstd [B] of the LayerNorm for the backward.  workspace: pm_pool_norm_workspace bytes.
 * pm_pool_norm_bwd: from dfeat [B, D]: dpooled = LayerNorm backward on the pooled row; dx[b, 0, :] = 0, dx[b, n >= 1, :] =
 *   dpooled[b] / (N - 1), written as f32 dx [B, N, D] and as its copy dx_act in act_dtype (round to nearest even; PM_F32: a second
 *   f32 copy), one coalesced pass of 16-byte stores.  dx NULL: not computed (dx_act must be NULL too); dx_act NULL: f32 only.
 *   dgamma[d] += sum_b dfeat xhat, dbeta[d] += sum_b dfeat, b ascending, ONE addition into what they held (accum_iter; the caller
 *   zeroes them for a fresh gradient); NULL: the parameter is frozen, nothing is written.  N >= 2, D % 4 == 0, D <= 2048,
 *   B <= 65535.  workspace: pm_pool_norm_bwd_workspace bytes.
 *
 * pm_linear_head_fwd: logits [B, C] = feat [B, D] W^T + bias, W [C, D].  D % 4 == 0, B, C <= 65535; logits / bias 4-byte aligned.
 * pm_linear_head_dfeat: dfeat [B, D] = dlogits [B, C] W, summed over c in ascending order.  dlogits 4-byte aligned.
 *   (dW / dbias of this head: pm_probe_head_bwd with feat as xhat.) */
typedef struct pm_mix_record {
  float lam;
  float one_minus_lam;
  int use_cutmix;
  int yl, yh, xl, xh;
  int reserved;
} pm_mix_record;
int pm_mix_batch(float* x, int B, int C, int H, int W, const pm_mix_record* rec, int enabled, void* stream);
int pm_soft_ce_workspace(int B, size_t* bytes);
int pm_soft_ce(const float* logits, const long long* target, int B, int C, const pm_mix_record* rec, float smoothing,
               const float* scale, float* loss, float* dlogits, void* workspace, size_t ws_bytes, void* stream);
int pm_pool_norm_fwd_train(const float* x, int B, int N, int D, const float* gamma, const float* beta, float eps, float* feat,
                           float* pooled, float* mean, float* rstd, void* workspace, size_t ws_bytes, void* stream);
int pm_pool_norm_bwd_workspace(int B, int N, int D, size_t* bytes);
int pm_pool_norm_bwd(const float* dfeat, const float* pooled, const float* mean, const float* rstd, const float* gamma, int B, int N,
                     int D, float* dx, void* dx_act, int act_dtype, float* dgamma, float* dbeta, void* workspace, size_t ws_bytes,
                     void* stream);
int pm_linear_head_fwd(const float* feat, int B, int D, int C, const float* W, const float* bias, float* logits, void* stream);
int pm_linear_head_dfeat(const float* dlogits, const float* W, int B, int D, int C, float* dfeat, void* stream);

/* ---- stochastic depth of the fine-tune ViT (pm_droppath.hip; timm 0.4.12 DropPath, mae/main_finetune.py:251 drop_path_rate) ----
 * A block's residual branches become x = x + s[b] * f(LN(x)) with one f32 scale per sample and branch.  Scale tables are f32, one
 * entry per sample; row r of an [M = B N, D] tensor belongs to sample r / N.  Any finite scale is taken, not only {0, 1 / keep}.
 * D % 4 == 0, M % N == 0, tensors 16-byte aligned.  No float atomics: results are run-to-run identical.
 *   pm_drop_path_add:        out[r,:] = x[r,:] + scale[r / N] * y[r,:] in f32, the product rounded before the sum (the bits of
 *                            torch's `x + y * s[:, None]`).  out may be y (in place on the buffer a GEMM just wrote).
 *   pm_drop_path_scale_cast: dy_act[r,:] = cast(scale[r / N] * dy[r,:]) to act_dtype (PM_BF16 / PM_F16 / PM_F32, round to nearest
 *                            even); colsum (optional, f32 [D]) += sum_r scale[r / N] * dy[r,:] through partial rows in `workspace`
 *                            (pm_drop_path_workspace(M, D) bytes, 16-byte aligned; a smaller one is refused when colsum is given),
 *                            summed in a fixed order.
 *   pm_drop_path_scales:     noise f32 [depth, 2, B] of U[0, 1) (pm_mae_noise), rates f32 [depth] (drop probability per block, on
 *                            the device) -> out[i, j, b] = fl32(keep_i + noise) >= 1 ? fl32(1 / keep_i) : 0 with keep_i =
 *                            fl32(1 - rates[i]); a block at rate 0 gets exactly 1.0 everywhere. */
int pm_drop_path_add(const float* x, const float* y, float* out, const float* scale, int M, int N, int D, void* stream);
int pm_drop_path_workspace(int M, int D, size_t* bytes);
int pm_drop_path_scale_cast(const float* dy, const float* scale, void* dy_act, int act_dtype, float* colsum, int M, int N, int D,
                            void* workspace, size_t ws_bytes, void* stream);
int pm_drop_path_scales(const float* noise, const float* rates, float* out, int depth, int B, void* stream);

/* ---- timm's RandAugment and random erasing of the MAE fine-tune transform (pm_timm_aug.hip; mae/util/datasets.py:37-47:
 * create_transform(auto_augment='rand-m9-mstd0.5-inc1', interpolation='bicubic', re_prob=0.25, re_mode='pixel')) ----
 * One LAYER of the policy = one op per sample on u8 [B][H][W][3] frames, src != dst.  ops points at the layer's first record,
 * sample b reads ops[b * stride] (a [B][n] plan is uploaded once: layer l is ops + l, stride n).  Every op restates the Pillow
 * routine timm calls, byte for byte (tests/randaug_ref.py pins them to Pillow 12.2):
 *   op  0 identity (a layer the op's probability skipped; posterize with 8 bits): copy
 *       1 AutoContrast   ImageOps.autocontrast, cutoff 0        \  need the three 256-bin histograms of the sample
 *       2 Equalize       ImageOps.equalize                      /
 *       3 Invert   4 Posterize(iarg bits, 0..7)   5 Solarize(iarg threshold)   6 SolarizeAdd(iarg, threshold 128): point tables
 *       7 Color   8 Contrast   9 Brightness   10 Sharpness: ImageEnhance, Image.blend(degenerate, image, farg) in C float, clipping
 *         when farg is outside [0, 1]; Contrast needs the sample's luminance sum; Sharpness blends against ImageFilter.SMOOTH
 *      11 Affine: Image.transform(size, AFFINE, a, BICUBIC, fillcolor): source point (a0 (x + .5) + a1 (y + .5) + a2, a3 .. a5) in
 *         double, Geometry.c bicubic_filter32RGB; where it lies outside the frame the pixel is (fill_r, fill_g, fill_b).
 *         ShearX / ShearY / TranslateX / TranslateY / Rotate all arrive as their matrix (Image.rotate's is built by the caller)
 *      12 Transpose: iarg 2 = ROTATE_180, 3 = ROTATE_90, 4 = ROTATE_270 (H == W), Image.rotate's early returns
 *   pm_randaug_stats: one workgroup per sample whose op is 1, 2 or 8 writes stats[b] (pm_randaug_workspace(B) bytes in all, 8-byte
 *     aligned: per sample 768 u32 bins + the u64 luminance sum); the caller skips the launch when no sample needs it.  Integer
 *     atomics in LDS only.
 *   pm_randaug_apply: hflip (u8 [B], optional; the first layer only) mirrors the SOURCE frame before the op -- timm flips before
 *     the policy.  stats may be NULL when no sample's op is 1, 2 or 8 (the caller knows its plan; a sample whose op needs
 *     statistics that were not given is copied).  Records are device memory and are trusted as the other tables are; reads stay inside frame b and writes inside
 *     dst whatever they hold (an unknown op copies).
 * pm_random_erase_f32: in place on the normalised f32 [B][C][H][W].  boxes i32 [B][max_count][4] = (top, left, h, w); h <= 0 or
 *   w <= 0: no box; a box that leaves the frame is skipped.  mode 0: zeros; 1: one normal per channel and box; 2: one per element.
 *   The normal of element e (mode 2: e = (c h + y) w + x inside the box; mode 1: e = c) of box k of sample b is Box-Muller over
 *   words of Philox4x32-10(counter = (e / 4, b max_count + k, counter lo, counter hi), key = seed lo, hi): words (0, 1) serve
 *   e % 4 = 0 (cos) and 1 (sin), words (2, 3) serve 2 and 3; u1 = ((w >> 8) + 1) 2^-24, u2 = (w' >> 8) 2^-24, z = sqrt(-2 ln u1)
 *   cos / sin(2 pi u2) in f32.  Where boxes of one sample overlap the later box holds, as in timm's loop.  Outside the boxes no
 *   byte is written.  mode 3 writes the uniforms themselves where mode 2 writes a normal (u1 for an even e, u2 for an odd one:
 *   exact 24-bit values), so that a test can hold the words to a host Philox with ==. */
typedef struct pm_randaug_op {
  int op, iarg;
  float farg;
  int reserved;
  double a[6];
} pm_randaug_op;
int pm_randaug_workspace(int B, size_t* bytes);
int pm_randaug_stats(const unsigned char* src, const pm_randaug_op* ops, int stride, void* stats, size_t stats_bytes, int B, int H,
                     int W, void* stream);
int pm_randaug_apply(const unsigned char* src, unsigned char* dst, const pm_randaug_op* ops, int stride, const unsigned char* hflip,
                     const void* stats, size_t stats_bytes, int B, int H, int W, int fill_r, int fill_g, int fill_b, void* stream);
int pm_random_erase_f32(float* x, const int* boxes, int max_count, int mode, unsigned long long seed, unsigned long long counter,
                        int B, int C, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif
