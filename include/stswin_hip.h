/* libstswin_hip -- C ABI of the MI355X-native STswinCL hot path.
 *
 * The reference (YuemingJin/STswinCL) is pure Python: its "operator interface" for this path is the
 * nn.Module surface; there is no FFI table to mirror.  This header is therefore the
 * boundary a maintainer binds with ctypes: plain device pointers, sizes and a
 * hipStream_t, no torch types.  Each entry point names the reference lines it replaces
 * (paths relative to the reference repo root).
 *
 * Conventions
 *   dtype      0 = bf16 storage (fp32 accumulate), 1 = fp32 storage (exact fp32 MFMA; parity path)
 *   pointers   device memory on the current HIP device; row pitches (ld*) in ELEMENTS
 *   row maps   int32, -1 = zero row (padding); NULL = identity
 *   stream     hipStream_t (pass torch.cuda.current_stream().cuda_stream); kernels are asynchronous
 *   return     0 on success, negative on error (-hipError_t, or -1xxx for argument errors)
 *   No entry point allocates, synchronises or keeps state: all workspaces are caller-owned.
 */
#ifndef STSWIN_HIP_H
#define STSWIN_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

/* gemm_nt epilogue flags */
#define STSWIN_GF_GELU 1       /* out = gelu_erf(v); C2 (if given) receives v            (swin_512.py:18-19) */
#define STSWIN_GF_RESID 2      /* v += R[r_rows[m]][n]                                   (swin_512.py:234-235) */
#define STSWIN_GF_MUL_DGELU 4  /* v *= gelu'(R[..])   (backward of swin_512.py:19) */
#define STSWIN_GF_OUT_F32 8    /* C is fp32 regardless of dtype */
#define STSWIN_GF_ACCUM 16     /* C += v (needs OUT_F32) */
#define STSWIN_GF_RELU 32
#define STSWIN_GF_MUL_R 8192     /* v *= R[r_rows[m]][n]  (R = GELU' values saved by STSWIN_GF_C2_DGELU) */
#define STSWIN_GF_C2_DGELU 16384 /* with GF_GELU: C2 receives gelu'(v) instead of v - the fc1 forward then hands the backward
                                    its multiplier and the backward epilogue is one multiply */
#define STSWIN_GF_CS_PARTIAL 32768 /* `colsum` is a caller-owned fp32 table [2*ceil(M/256)][N] instead of the fp32 [N] accumulator: row b
                                    * receives (plain stores, no atomics) the column sums of output rows 128b..128b+127;
                                    * stswin_cs_reduce then adds the rows into the bias gradient.  M/128 same-address atomics cost
                                    * 38 us on a 65536 x 512 output; the table + reduce cost ~5 us (N % 4 == 0).
                                    * Kernels whose workgroups own 256 output rows without a 128-row split (the 256x64 tiles, the 256x256 ring with
                                    * the fp32 LDS epilogue) store the sum of rows 256t..256t+255 in row 2t and zero in row 2t+1: every consumer
                                    * (stswin_cs_reduce, stswin_cs_group_reduce) works on whole 256-row tiles (tests/test_hip_gemm_nt_contract.py). */
#define STSWIN_GF_CS_SQ 65536   /* with STSWIN_GF_CS_PARTIAL: `colsum` holds TWO planes [2][2*ceil(M/256)][N]; the second receives the column
                                  * sums of SQUARES of the same values: the BatchNorm statistics of a convolution output come out of
                                  * the convolution (stswin_cs_group_reduce + stswin_bn_finalize with x = NULL) */
#define STSWIN_GF_TAPSKIP (1 << 29) /* tiled (non-ring) kernels, S > 1 with a_rows: a workgroup first scans its rows of the map and skips every
                                    * segment (convolution tap) that is padding for ALL of them - pays when every row tile has such a tap (dilation >=
                                    * half the map height: ASPP's dilation 18 on 32 x 32: 70 -> 53 us); the scan costs ~4 us per launch.
                                    * Bitwise neutral for FINITE weights only: a skipped all-padding tap contributes 0 * w, which the unskipped
                                    * kernel evaluates as NaN when w is Inf / NaN - a diverged run can look healthy in the skipped taps */
#define STSWIN_GF_BIG 128       /* tuning: force the 256x256 4-stage-ring kernel (bf16) */
#define STSWIN_GF_MID 512       /* tuning: 256x128x32 tile, 3-stage ring, 2 workgroups per CU (bf16) */
#define STSWIN_GF_NOPIPE 1024   /* tuning: 256x256 ring kernel without software-pipelined LDS fragment reads */
#define STSWIN_GF_HALF 2048     /* tuning: force the 256x128 ping-pong ring kernel */
#define STSWIN_GF_M32PP (1u << 31) /* tuning (STSWIN_TUNING builds): the 8-wave ping-pong ring on 32x32x16 MFMA tiles; with STSWIN_GF_W4R: the 4-wave
                                  * register-staged variant (global_load + ds_write_b128 instead of LDS-DMA).  All measured slower: profiles/r04_gemm_w4_experiment.txt */
#define STSWIN_GF_W4R (1 << 30) /* tuning (STSWIN_TUNING builds only): 256x256 ring with 4 waves of 128x128, one per SIMD, register-pipelined
                                 * 32x32x16 main loop - the vendor kernel's structure; same results, measured slower (profiles/r04_gemm_w4_experiment.txt) */
#define STSWIN_GF_ROT 4096      /* tuning (STSWIN_TUNING builds): 256x256 ring with the rotated ping-pong loop, one barrier per stage */
#define STSWIN_GF_NOBIG 256     /* tuning: forbid it (default: chosen when >= 256 big tiles fill the chip) */
#define STSWIN_GF_WAVES4 64     /* tuning: 4 waves of 64x64 per 128x128 tile instead of the default 8 waves of 64x32 */
#define STSWIN_GF_NOREGEPI (1 << 22) /* tuning: 256x256 ring with the LDS-staged fp32 epilogue instead of the register epilogue */
#define STSWIN_GF_NOSTREAM (1 << 23) /* tuning: 256x256 ring without the persistent streaming variant */
#define STSWIN_GF_DUO (1 << 24)      /* tuning: 128x256 tiles, 4 waves, two workgroups per CU */
#define STSWIN_GF_STREAM (1 << 25)   /* tuning: persistent streaming 256x256 variant (measured no faster: both wave rows idle through each other's epilogue) */
#define STSWIN_GF_NONARROW (1 << 26) /* tuning: forbid the 256x64 tile for N <= 64 */
#define STSWIN_GF_NODEEP (1 << 27)   /* tuning: the 128x64 few-tiles kernel with its double buffer instead of the 4-stage ring */
#define STSWIN_GF_DEEP (1 << 28)     /* tuning: 3-stage rings for the 128x128 / 256x64 kernels too (one workgroup per CU) */

int stswin_abi_version(void);

/* ---- a1-a4: roll + window_partition + pair regroup, and its inverse ------------------------------------
 * swin_512.py:26-38 (window_partition), :57-71 (window_reverse, T-aware), :210-218, :224-231 (roll, regroup).
 * Tokens are rows of a (B, frames_total, H*W, C) tensor; the pair is frames f0..f0+T-1 of every clip.
 * win_rowmap writes map[r] = source token of gathered row r (row order (B*nW, T, ws*ws));
 * win_move copies rows: dir 0 gather (out[r] = in[map[r]]), dir 1 scatter (out[map[r]] = in[r]). Bit-exact. */
int stswin_win_rowmap(int* map, int B, int T, int H, int W, int ws, int shift, int f0, int frames_total, void* stream);
int stswin_win_move(int dtype, const void* in, void* out, int B, int T, int H, int W, int C, int ws, int shift,
                    int f0, int frames_total, int dir, void* stream);
/* PatchMerging 2x2 gather map, 4 segments in the order (0,0),(1,0),(0,1),(1,1)  (swin_512.py:267-271). */
int stswin_merge_rowmap(int* map /*[4][frames*H/2*W/2]*/, int frames, int H, int W, void* stream);
/* 3x3 convolution tap map (padding = dilation), 9 segments ky*3+kx   (ASPP.py:13-20, base18.py:73). */
int stswin_conv3x3_rowmap(int* map /*[9][frames*H*W]*/, int frames, int H, int W, int dilation, void* stream);
/* general k x k convolution tap maps (resnet.py:31-34: stride 1/2, dilation 1/2/4; torchvision stem layers):
 * inverse = 0: map[t][m_out] = input pixel read by output pixel m_out through tap t (or -1 = padding);
 * inverse = 1: map[t][n_in]  = the output pixel that reads input pixel n_in through tap t (or -1)  -> dgrad gather. */
int stswin_conv_rowmap(int* map, int frames, int Hin, int Win, int Hout, int Wout, int k, int stride, int pad, int dilation,
                       int inverse, void* stream);
/* stem im2col (torchvision conv1 7x7/2 pad 3, Cin = 3; resnet.py:102): NCHW fp32 images [F][3][H][W] ->
 * patches [F*Ho*Wo][ld] with column (ky*7+kx)*3 + c, zero padded to ld. */
int stswin_stem_im2col(int dtype, const float* img, void* patches, long ld, int frames, int H, int W, int Ho, int Wo,
                       void* stream);
/* stem input as a 2 x 2 space-to-depth image (torchvision conv1 7x7/2 pad 3 = a 4 x 4 / stride 1 convolution over 12-channel
 * superpixels; resnet.py:98-102): NCHW fp32 images [F][3][H][W] -> records [F][Ho + 3][Wo + 3][16] (Ho = (H-1)/2 + 1; 2 records of
 * zero padding before, 1 after, in both directions), record (sy, sx)[(dy*2 + dx)*3 + c] = img[c][2(sy-2) + dy][2(sx-2) + dx],
 * positions 12..15 zero.  Output pixel (oy, ox) contracts, per tap row s = 0..3, the 64 contiguous values of records
 * (oy + s, ox .. ox + 3) with W[co][c][2s + dy - 1][2t + dx - 1] (t = record in the segment; taps outside 0..6 are zero):
 * stswin_gemm_nt / stswin_gemm_tn with a row map [4][M], Kseg = bseg = 64 and lda = 16.  The buffer must extend 48 values past
 * the last record (the last segment reads on). */
int stswin_stem_s2d(int dtype, const float* img, void* out, int frames, int H, int W, void* stream);
/* The stem convolution over the space-to-depth image `rec` of stswin_stem_s2d (bf16): y bf16 [F*Ho*Wo][64] = conv(7, 2, 3) with
 * wmat bf16 [64][4][4][16] (= [cout][tap row][record][position], zeros where the 7 x 7 window has no tap); stats (or NULL): a
 * STSWIN_GF_CS_SQ table ([2][2*ceil(M/256)][64]) of the fp32 values BEFORE the bf16 store, written per RUN: a workgroup takes `per`
 * consecutive units (unit = one output row of a 128-pixel-wide strip = one 128-row block), a run ends with the workgroup's units or
 * with the strip; the row of a run's FIRST block holds the sums | sums of squares of the whole run, the rows of its other blocks hold
 * 0.0.  Every row up to M/128 is written; consumers must add the rows of whole frames (stswin_cs_group_reduce and
 * stswin_bn_table_finalize over groups of whole frames), a single row is not the sum of its own block.  Record rows pass through an LDS ring once, the weights live in registers:
 * replaces stswin_gemm_nt over the row map for this M = F*Ho*Wo, N = 64, K = 256 shape.  Wo % 128 != 0: -1732, nothing launched.
 * resnet.py:98-102.  Per-element contract (this kernel, stswin_stem_wgrad, stswin_conv3x3_c64 and stswin_conv3x3_c64_wgrad):
 * tests/conv_halo_ref.py, tests/test_conv_halo_ref.py, tests/test_hip_conv_halo_contract.py. */
int stswin_stem_conv(const void* rec, const void* wmat, void* y, float* stats, int frames, int H, int W, void* stream);
/* Weight gradient of the stem convolution from dy (bf16 [F*Ho*Wo][64]) and the space-to-depth image `rec` of stswin_stem_s2d (bf16):
 * dw fp32 [64][4][4][16] = [cout][tap row][record][position], the order stswin_gemm_tn produces over the row map (accumulate != 0 adds).
 * Record rows pass through an LDS ring once; per-workgroup partials go to `scratch` (>= stswin_stem_wgrad_scratch floats) and are added
 * in a fixed order.  Wo = (W-1)/2 + 1 must be a multiple of 128, else -1722 and nothing is launched.  resnet.py:98-102 backward. */
long stswin_stem_wgrad_scratch(int frames, int Ho, int Wo);
int stswin_stem_wgrad(const void* dy, const void* rec, float* dw, int accumulate, float* scratch, long scratch_floats, int frames, int H, int W,
                      void* stream);
/* (Cout, Cin, k, k) fp32 nn.Conv2d weight -> the bf16 / fp32 GEMM operand matrices of the token convolutions in one launch:
 * fwd [cop][S][cip] (tap-major K of stswin_gemm_nt) and, if not NULL, dgrad [cip][S][cop].  omap[cop] / imap[cip] = source
 * channel of each padded channel position or -1 (zero).  (ASPP.py:37-50, base18.py:60-77, resnet.py convolutions) */
int stswin_conv_pack(int dtype, const float* w, void* fwd, void* dgrad, const int* omap, const int* imap, int co, int ci, int S,
                     int cop, int cip, void* stream);
/* nn.Linear weight [n][k] fp32 -> fwd [n][k] and (if not NULL) tr [k][n] in the compute dtype, one launch (n, k multiples of 4):
 * the B operands of y = x W^T and of dx = dy W (swin_512.py:18-21,115,139,275), re-made after every optimizer step. */
int stswin_linear_pack(int dtype, const float* w, void* fwd, void* tr, int n, int k, void* stream);
/* The same two packings for up to 64 Linear / 32 convolution weights in ONE launch each (host arrays of device pointers and
 * sizes): the re-cast of every GEMM operand after an optimizer step (train_swin.py:170-173 steps ~125 M parameters) was ~90
 * launches of 6-15 us; see stswincl_amd.ops.repack. */
int stswin_linear_pack_multi(int dtype, int count, const float* const* w, void* const* fwd, void* const* tr, const int* n, const int* k,
                             void* stream);
int stswin_conv_pack_multi(int dtype, int count, const float* const* w, void* const* fwd, void* const* dgrad, const int* const* omap,
                           const int* const* imap, const int* ci, const int* S, const int* cop, const int* cip, void* stream);
/* nn.MaxPool2d(3, 2, 1) on tokens [F][H][W][C] -> [F][Ho][Wo][C]; arg (uint8 [F*Ho*Wo][C]) = winning tap (first max in
 * (ky,kx) scan order, like torch); backward gathers dy through arg (no atomics). */
int stswin_maxpool3x3s2(int dtype, const void* in, long ldi, void* out, long ldo, unsigned char* arg, int frames, int H,
                        int W, int Ho, int Wo, int C, int backward, void* stream);
/* 3x3 / stride 1 / pad 1 convolution of 64 -> 64 channels over bf16 NHWC tokens [frames*H*W][64] (torchvision resnet18.layer1 as
 * used by resnet.py:104-105, basic blocks resnet.py:31-51) from an LDS-resident halo with the weights in registers: replaces the
 * gather form of stswin_gemm_nt for these shapes.  wmat = the [64][9][64] matrices stswin_conv_pack makes; sign = +1 with the fwd
 * matrix: the convolution; sign = -1 with the dgrad matrix: its input gradient (x = dy).  resid (or NULL): [frames*H*W][64] added
 * before the store (a gradient another consumer of the input produced); stats (or NULL): the STSWIN_GF_CS_SQ table
 * ([2][2*ceil(M/256)][64]: per-128-row-block column sums | sums of squares) of the fp32 values BEFORE the bf16 store (residual
 * included), not of the stored bf16 values; every row is written, also when workgroups are left without a tile.  W in {16, 32, 64,
 * 128}, H*W % 256 == 0; other geometries return -1702 / -1701 and launch nothing (the caller keeps the gather GEMM).  Per-element
 * contract: tests/conv_halo_ref.py, tests/test_conv_halo_ref.py, tests/test_hip_conv_halo_contract.py. */
int stswin_conv3x3_c64(const void* x, const void* wmat, void* y, const void* resid, float* stats, int frames, int H, int W, int sign,
                       void* stream);
/* Weight gradient of the same convolution from dy and x (both bf16 [frames*H*W][64]): dw fp32 [64][9][64] (the order of
 * stswin_gemm_tn with bseg = 64: [cout][tap][cin]) or, tapminor != 0, [64][64][3][3] (nn.Conv2d.weight's own layout); accumulate != 0
 * adds to dw instead of overwriting it.  Image rows of x pass through an LDS ring once, per-workgroup partials go to `scratch`
 * (>= stswin_conv3x3_c64_wgrad_scratch(frames, H, W) floats) and are added in a fixed order: bitwise reproducible.  W in {32, 64,
 * 128}, H*W % 128 == 0; else -1712 / -1711 and nothing is launched (the caller keeps stswin_gemm_tn).  resnet.py:31-51 backward. */
long stswin_conv3x3_c64_wgrad_scratch(int frames, int H, int W);
int stswin_conv3x3_c64_wgrad(const void* dy, const void* x, float* dw, int tapminor, int accumulate, float* scratch, long scratch_floats,
                             int frames, int H, int W, void* stream);

/* ---- segmented gather GEMM: C[c_rows[m]][n] = epi( sum_s A[a_rows[s][m]][0:Kseg] . B[n][s*Kseg:(s+1)*Kseg] )
 * nn.Linear of swin_512.py:115 (qkv, with the window gather fused via a_rows and the q scaling via
 * scale/scale_cols, :118), :139 (proj, with window_reverse + un-roll + shortcut fused via c_rows/r_rows, :224-234),
 * :18-21 (Mlp fc1+GELU, fc2 + residual), :275 (PatchMerging reduction); 1x1 / 3x3 / dilated nn.Conv2d of
 * ASPP.py:37-50 and base18.py:60-77 as implicit GEMM over NHWC tokens.  Kseg must be a multiple of 64 (bf16) / 32 (f32). */
int stswin_gemm_nt(int dtype, const void* A, long lda, const int* a_rows, const void* B, long ldb, void* C, long ldc,
                   const int* c_rows, void* C2, long ldc2, const float* bias, const void* R, long ldr,
                   const int* r_rows, int M, int N, int Kseg, int S, float scale, int scale_cols, int flags,
                   float* colsum /* optional fp32 [N]: += column sums of the stored values (bias gradient) */, void* stream);
/* out[n] += sum_b partials[b][n], b < 2*ceil(M/256): second half of a STSWIN_GF_CS_PARTIAL stswin_gemm_nt (same M, N). */
int stswin_cs_reduce(const float* partials, int M, int N, float* out, void* stream);
/* weight gradients: C[i][j] += sum_m At[at_rows[m]][i] * Bt[bt_rows[m]][j]   (fp32 atomics; splits<=0: auto).
 * bseg > 0 (convolution wgrad in one launch): column j of the B operand is column j % bseg of row
 * bt_rows[(j / bseg) * Mk + m], i.e. tap t = j / bseg uses its own row map.
 * With bf16 operands and a workspace the split-K partials are kept as bf16 (each an fp32 sum of Mk / splits products, rounded
 * once; the combine pass adds them in fp32): half the slab traffic.  Environment STSWIN_TN_F32_SLABS=1 keeps fp32 partials.
 * Bits of a positive `splits`: STSWIN_TN_OVERWRITE (1<<27) stores C = result instead of accumulating (C may be
 * uninitialised; saves the caller's zero fill); bits 28-30 are tuning overrides (forbid / force the 256x256 ring kernel,
 * 4-wave 128x128 variant) used by tools/tn_sweep.py; the low bits are the split count, 0 = automatic. */
#define STSWIN_TN_OVERWRITE (1 << 27)
#define STSWIN_TN_NO_COMBINE (1 << 26)   /* with a workspace: leave the partials there; the caller runs stswin_tn_combine */
/* gemm_nt for few output tiles and a long K (ASPP.py:13-20,37-40: dilated 3x3 convolutions on 32x32 maps; M = 4096, N = 512,
 * K = 9 x 1024): the 256x256 ring kernel over tiles x K-splits with fp32 partial slabs in `workspace`, then a fixed-order combine
 * (+ bias, ReLU) into C (bf16, pitch ldc).  bf16 only, plain epilogue only.  stswin_gemm_nt_splitk_scratch returns the floats of
 * workspace needed, or 0 when the shape is not a candidate (<= 32 tiles of 256x256, >= 64 stages of 32: call stswin_gemm_nt).
 * Environment STSWIN_SPLITK_BF16=1 (tuning, read per call): bf16 partial slabs - 20 % faster, the partials rounded once more. */
long stswin_gemm_nt_splitk_scratch(int M, int N, int Kseg, int S);
int stswin_gemm_nt_splitk(const void* A, long lda, const int* a_rows, const void* B, long ldb, void* C, long ldc, const float* bias, int M, int N,
                          int Kseg, int S, int relu, float* workspace, long workspace_floats, void* stream);
/* Fused split-K combine (the default where it applies; stswin_last_variant(1) then carries STSWIN_VAR_TN_FUSED): with bf16 operands, a
 * workspace, the 256x256 ring kernel and a grid of at most one workgroup per compute unit, the partial tiles are combined INSIDE the
 * launch - every workgroup of a tile signals an arrival counter; once the tile's partials are complete its row slices are handed out by
 * ticket to the workgroups of the tile that are present and added in split order (bit for bit the separate pass's result;
 * tests/test_hip_gemm.py).  No workgroup depends on another one being resident: an early workgroup polls for a bounded time
 * (200 us) and then leaves, the last arriver takes whatever slices are left - a second stream, a second process or an RCCL kernel
 * holding compute units costs time, never correctness, and nothing traps.  Counter regions are per (device, stream).
 * stswin_tn_fused_hold(+1 / -1 / 0) adds / releases / reads a process-wide hold: while any hold is outstanding the separate
 * tn_reduce pass is used (GradBucketReducer holds one while its collectives overlap backward); environment STSWIN_TN_FUSED=0 / 1
 * overrides the holds (read per call). */
int stswin_tn_fused_hold(int delta);
/* Compute units the one-workgroup-per-CU launches plan for (split-K factor of the gemm_tn ring kernel, persistent grids of the attention
 * backward): the whole device (256) by default; lower it while a communication kernel is known to hold k units (256 - k), 0 restores
 * the default.  Returns the previous setting.  A planning hint only: any value gives correct results. */
int stswin_set_cu_budget(int cus);
int stswin_gemm_tn(int dtype, const void* At, long lda, const int* at_rows, const void* Bt, long ldb, const int* bt_rows,
                   float* C, long ldc, int Mk, int Ni, int Nj, int splits, int bseg,
                   float* workspace /* optional caller-owned scratch: split-K partials are stored there and combined by a
                                       second kernel instead of fp32 atomics */, long workspace_floats, void* stream);
/* Up to 4 bf16 weight-gradient problems of ONE backward step in one launch (round 5).  The reference's autograd computes the weight
 * gradients of a Swin block one by one (swin_512.py:115-141,18-21 through torch.autograd: qkv, proj, fc1, fc2); each of those GEMMs has
 * few 256x256 output tiles (4-16 at stage 1), so alone it needs 16-64 contraction splits to fill the device and pays its own ramp,
 * partial-tile round trip and combine.  Launched together, the three that are ready at the end of a block's backward (fc1, proj, qkv)
 * are 32 tiles x 8 splits = 256 workgroups.  Every problem is one stswin_gemm_tn would give to the 256x256 ring kernel with the fused
 * combine (both output dims >= 256, at most one row map, bf16 partials, ldc >= 0); split counts are chosen so that every workgroup
 * gets about the same number of 32-row stages and the grid is at most one workgroup per compute unit (stswin_set_cu_budget).
 * Returns 0 when launched; STSWIN_TN_GROUP_DECLINED when the set is not eligible (a hold of stswin_tn_fused_hold is outstanding,
 * STSWIN_TN_FUSED=0 / STSWIN_TN_F32_SLABS=1 / STSWIN_TN_GROUP=0 in the environment, a shape outside the ring kernel's range, less than
 * 7/8 of the device filled, workspace too small) - nothing has been written and the caller launches the problems one by one with
 * stswin_gemm_tn; other negative codes: malformed arguments.  splits_out (optional, [count]): the split counts used.  The result of a
 * problem is a deterministic function of its operands and its split count (partials rounded to bf16 once, added in split order). */
#define STSWIN_TN_GROUP_DECLINED (-1050)
typedef struct stswin_tn_problem {
  const void* At; long lda; const int* at_rows;     /* [Mk (gathered by at_rows)][Ni] */
  const void* Bt; long ldb; const int* bt_rows;     /* [Mk (gathered by bt_rows; with bseg > 0: per-tap maps [Nj / bseg][Mk])][Nj or bseg] */
  float* C; long ldc;                               /* [Ni][Nj] fp32 */
  int Mk, Ni, Nj, bseg;
  int overwrite;                                    /* 1: C = result, 0: C += result */
  int tapminor;                                     /* with bseg > 0: store [row][channel][tap] (STSWIN_TN_OUT_TAPMINOR) */
} stswin_tn_problem;
int stswin_gemm_tn_group(int dtype, int count, const stswin_tn_problem* problems, float* workspace, long workspace_floats, int* splits_out,
                         void* stream);
/* The combine pass of a stswin_gemm_tn launched with STSWIN_TN_NO_COMBINE, for callers that run it on a second stream (it then
 * overlaps the input-gradient GEMM that follows every weight-gradient GEMM of a backward pass instead of standing between two
 * launches; ordering between the two streams is the caller's: events).  splits / slab_bf16 as stswin_last_variant(1) reported
 * them for that launch (no partials were written if it reported no slab bit: nothing to combine, C is final). */
int stswin_tn_combine(const float* workspace, float* C, long ldc, int Ni, int Nj, int splits, int overwrite, int slab_bf16,
                      void* stream);
/* Which kernel the launcher chose for the calling thread's most recent stswin_gemm_nt (family 0) / stswin_gemm_tn
 * (family 1) call: one of the codes below (family 1: | slab bits | split count << 16).  Test instrumentation only - the
 * parity suite asserts that the production shapes of the training step run the production kernels
 * (swin_512.py:109-141 qkv/proj, :7-23 Mlp, resnet.py:31-34 3x3 convolutions and their weight gradients), and the float64
 * contracts assert the word per kernel and per combine form: tests/test_hip_gemm_nt_contract.py for family 0,
 * tests/test_hip_gemm_tn_contract.py for family 1 (the whole word: kernel code, slab type, fused, tap-minor, split count). */
#define STSWIN_VAR_F32 100                 /* added to a 128x128-family code when the exact-fp32 instantiation ran */
#define STSWIN_VAR_NT_RING256_REGEPI 1     /* 256x256 ping-pong ring, operand-swapped MFMA + register epilogue (production) */
#define STSWIN_VAR_NT_RING256_LDSEPI 2     /* 256x256 ping-pong ring, fp32 LDS epilogue (fp32 outputs, unaligned operands) */
#define STSWIN_VAR_NT_RING256_NOPIPE 3
#define STSWIN_VAR_NT_RING256_W4 14        /* 256x256 ring, 4 waves of 128x128, register-pipelined main loop (GF_W4R / STSWIN_NT_W4=1) */
#define STSWIN_VAR_NT_STREAM 4
#define STSWIN_VAR_NT_DUO 5
#define STSWIN_VAR_NT_RING256x128_PP 6
#define STSWIN_VAR_NT_MID 7
#define STSWIN_VAR_NT_256x64 8
#define STSWIN_VAR_NT_128x64 9
#define STSWIN_VAR_NT_128x128 10
#define STSWIN_VAR_NT_128x128_W4 11
#define STSWIN_VAR_NT_SPLITK 13        /* 256x256 ring on tiles x splits + fp32 slab combine (stswin_gemm_nt_splitk); splits in bits 16.. */
#define STSWIN_VAR_NT_ROWS 12          /* M <= 8 rows: one wave per output column (ASPP.py:43-46 image-pool branch) */
#define STSWIN_VAR_TN_RING_PLAIN 20        /* gemm_tn_ring_kernel<0> */
#define STSWIN_VAR_TN_RING_ATROWS 21       /* <1> */
#define STSWIN_VAR_TN_RING_BTROWS 22       /* <2> */
#define STSWIN_VAR_TN_RING_BSEG 23         /* <3>: tap-segmented convolution weight gradient */
#define STSWIN_VAR_TN_128x128 30
#define STSWIN_VAR_TN_128x128_W4 31
#define STSWIN_VAR_TN_ROWS 32          /* Mk <= 8: a sum of outer products, no split-K slabs */
#define STSWIN_VAR_TN_SLABS_F32 0x1000     /* split-K partial slabs + tn_reduce, fp32 partials */
#define STSWIN_VAR_TN_SLABS_BF16 0x2000    /* ... bf16 partials */
#define STSWIN_VAR_TN_FUSED 0x8000         /* the split-K partials were combined inside the GEMM launch (no tn_reduce pass) */
#define STSWIN_VAR_TN_TAPMINOR 0x4000      /* the combine stored the result tap-minor (STSWIN_TN_OUT_TAPMINOR was honoured) */
#define STSWIN_TN_OUT_TAPMINOR (1 << 25)   /* bit of `splits` (with bseg > 0): store C[i][c * S + s] for GEMM column j = s * bseg + c, S = Nj / bseg - the [cout][cin][k][k]
                                            * layout of a convolution weight gradient; only where split-K slabs are combined (check stswin_last_variant) */
/* The QKV projection with an fp8 (OCP e4m3) result + one fp32 scale per (window problem, head of q / k / v): BASELINE.json configs[4]
 * ("fp8 MFMA attention"), swin_512.py:115-121 with q | k | v stored in 8 bits.  out8 [M][ld8] bytes, scales [M / rows_per_problem][ld_scales]
 * (column = n / head_dim: the heads of q, then of k, then of v); value = e4m3 byte * scale.  stswin_win_attn_fwd_f8 / _bwd_f8 read them. */
int stswin_gemm_nt_qkv_fp8(const void* A, long lda, const int* a_rows, const void* B, long ldb, void* out8, long ld8, float* scales,
                           long ld_scales, const float* bias, int M, int N, int Kseg, float scale, int scale_cols, int rows_per_problem,
                           int head_dim, void* stream);
/* Window attention on fp8-STORED q | k | v (stswin_gemm_nt_qkv_fp8's output): the core of swin_512.py:117-138 with both products on the fp8
 * MFMA, fp32 softmax; out bf16 [rows][ldo].  Geometries: (T ws^2, head dim) = (128, 128) and (32, 256) - the two stages of the model;
 * anything else returns -1201 (the caller keeps bf16 storage there). */
int stswin_win_attn_fwd_f8(const void* qkv8, long ld8, const float* scales, long ld_scales, void* out, long ldo, const float* biasT,
                           const float* maskT, int nB_, int nW, int T_frames, int ws, int heads, int C, int bias_windows,
                           const int* bias_index, void* stream);
/* ... and its backward: dqkv (bf16 [rows][lddq], the gradient of the dequantised q | k | v), dbiasT / dqkv_colsum as stswin_win_attn_bwd; scratch =
 * stswin_win_attn_bwd_scratch(nB_, ws, heads, C) floats.  Geometries: 8x8 windows x 2 frames x head dim 128, 4x4 x 2 x 256. */
int stswin_win_attn_bwd_f8(const void* qkv8, long ld8, const float* scales, long ld_scales, const void* dout, long lddo, void* dqkv, long lddq,
                           const float* biasT, const float* maskT, float* dbiasT, float* dqkv_colsum, int nB_, int nW, int T_frames, int ws,
                           int heads, int C, float scale, int bias_windows, const int* bias_index, float* scratch, long scratch_floats,
                           void* stream);
int stswin_last_variant(int family);
/* 1: the library was built with -DSTSWIN_TUNING (STSWIN_TUNING=1 python __graft_entry__.py --force) and holds the A/B-only gemm_nt variants
 * (STSWIN_GF_MID / _HALF / _NOPIPE / duo / stream: each measured slower than the default dispatch); 0: the product build, which ignores
 * those flags and picks the default kernel. */
int stswin_tuning_build(void);

/* ---- deterministic cross-workgroup sums.  No kernel of this library adds fp32 values with atomics any more: every kernel that sums
 * over workgroups (bias / LayerNorm / BatchNorm parameter gradients, BatchNorm statistics, the relative-position-bias gradient, the
 * OHEM statistics) stores one partial vector per workgroup ("slab") into caller-owned scratch and stswin_slab_fold's kernel adds the
 * slabs in a fixed order behind the launch boundary, so a training step gives the same bits every time it runs.  The `scratch`
 * arguments below are that space: uninitialised fp32, at least stswin_<entry>_scratch(...) floats, 16-byte aligned, private to the
 * call until the next kernel on the stream has run (one buffer per stream can serve every call).
 *   out_s[b*obs + j] (+)= sum_{p < nslabs} ws[b*ws_batch_stride + p*slab_stride + s*seg_len + j],  s < nseg <= 3, j < seg_len
 * The kernel loads and stores float4: ws, every non-NULL out_s and - in bytes - slab_stride, ws_batch_stride and out_batch_stride (obs) must
 * be 16-byte aligned, seg_len a multiple of 4 (-1110 where a length or a stride is not; the pointers are the caller's to keep aligned).  A NULL
 * out_s skips segment s.  nseg > 3: -1110; nseg <= 0, seg_len <= 0, nslabs <= 0 or batch <= 0: 0, nothing is written.  The association of the
 * sum depends on nslabs alone: 16 slab lanes (64 from nslabs = 96) each add every 16th (64th) slab in order, the lane sums are added in lane
 * order - the same bits whether the fold is launched at once or queued (below). */
int stswin_slab_fold(const float* ws, long slab_stride, long ws_batch_stride, int nslabs, int seg_len, int nseg, float* out0, float* out1,
                     float* out2, long out_batch_stride, int batch, int accumulate, void* stream);

/* stswin_fold_defer(1): from now on (calling thread) the folds of the entry points are QUEUED instead of launched - each call must
 * then get its own scratch region - and stswin_fold_flush launches them as one kernel; stswin_fold_defer(0) flushes and returns to
 * immediate folds.  Legal when no folded output is read before the flush (the backward of a Swin block: all parameter gradients). */
int stswin_fold_defer(int on, void* stream);
int stswin_fold_flush(void* stream);

/* out[n] += sum_m Y[m][n]  (bias gradients) */
long stswin_colsum_scratch(int M, int N);
int stswin_colsum(int dtype, const void* y, long ldy, float* out, int M, int N, float* scratch, void* stream);

/* ---- nn.LayerNorm (swin_512.py:160,166 norm1/norm2; :253,:274 PatchMerging.norm with the 2x2 gather fused:
 * row r = concat_s x[rows[s][r]][0:Cseg]).  mean/rstd (fp32 [M]) are saved for the backward; mean == NULL: neither is written.
 * A row lives in registers, 16 bytes per lane and piece.  Largest C = S*Cseg (beyond it -1104, or -1106 where the backward's (waves + 1) x C
 * fp32 LDS table would pass 64 KiB):      forward   bf16 8192   fp32 4096        backward   bf16 3272   fp32 2048
 * Cseg and every pitch must be a multiple of 16 bytes' worth of elements (8 bf16 / 4 fp32): -1105.  A NULL scratch: -1111. */
int stswin_layernorm_fwd(int dtype, const void* x, long ldx, const int* rows, int S, int Cseg, void* y, long ldy,
                         const float* gamma, const float* beta, float* mean, float* rstd, int M, float eps, void* stream);
int stswin_layernorm_bwd(int dtype, const void* dy, long lddy, const void* x, long ldx, const int* rows, int S, int Cseg,
                         const float* gamma, const float* mean, const float* rstd, void* dx, long lddx, float* dgamma,
                         float* dbeta, int M, int accumulate_dx,
                         float* dxsum /* optional fp32 [S*Cseg]: += column sums of dx (in the layout of dy: column s*Cseg + c of row r is
                                         what goes to dx[rows[s][r]][c]) taken from the fp32 values BEFORE they are rounded to the output type -
                                         with accumulate_dx, old + LN'(dy) in fp32.  In bf16 this is NOT the sum of the stored values: it is
                                         the better bias gradient of the Linear that produced x. */,
                         float* scratch /* >= stswin_layernorm_bwd_scratch(M, S*Cseg) floats: one [3][S*Cseg] slab (dgamma | dbeta |
                                           dxsum partial sums) per workgroup; folded into dgamma / dbeta / dxsum (+=) in slab order */,
                         void* stream);
/* The same with the accumulated-into tensor as a separate, read-only operand: dx = add + LN'(dy).  The backward of a pre-norm block
 * (swin_512.py:228-234: x = shortcut + attn; x = x + mlp(norm2(x))) then leaves the incoming gradient `add` intact for the weight-gradient
 * GEMM that reads it later (stswin_gemm_tn_group). */
int stswin_layernorm_bwd_add(int dtype, const void* dy, long lddy, const void* x, long ldx, const int* rows, int S, int Cseg,
                             const float* gamma, const float* mean, const float* rstd, const void* add, long ldadd, void* dx, long lddx,
                             float* dgamma, float* dbeta, int M, float* dxsum, float* scratch, void* stream);
long stswin_layernorm_bwd_scratch(int M, int C);

/* out[i] = map[i] >= 0 ? v[map[i]] : fill, i < n: padding of per-channel parameter vectors (BatchNorm weight / bias / running
 * statistics) to the 64-aligned channel layout of the token matrices and the gather back (base18.py:60-77 concat layout). */
int stswin_vec_gather(const float* v, const int* map, float* out, int n, float fill, void* stream);
/* the same for `count` (<= 4) vectors that share the map, in one launch: out[k][i] = map[i] >= 0 ? v[k][map[i]] : fill[k]
 * (v, out, fill: host arrays).  out[k] may be a parameter / buffer itself (the un-padded running statistics are written in place). */
int stswin_vec_gather_multi(int count, const float* const* v, const int* map, float* const* out, int n, const float* fill, void* stream);

/* ---- relative position bias (swin_512.py:122-131).  expand: out[w][h][j][i] = table[index[i*N + j]][h] (+ mask[w][i][j]),
 * the [key][query] layout of stswin_win_attn_fwd's biasT (nW = 1, mask = NULL: plain [heads][N][N]; with the SW-MSA mask the
 * per-window pre-summed table).  scatter: dtable[index[i*N + j]][h] += dbiasT[h][j][i] (the backward of the gather).
 * table / dtable fp32 [(2ws-1)^2][heads], index int64 [N*N] (the module's relative_position_index buffer). */
int stswin_bias_expand(const float* table, const long* index, const float* mask, float* out, int N, int heads, int nW,
                       void* stream);
/* the same for `count` (<= 16) tables in one launch (host arrays of device pointers / sizes; mask[e] may be NULL): every Swin block's
 * table right after an optimizer step instead of one launch per block forward */
int stswin_bias_expand_multi(int count, const float* const* table, const long* const* index, const float* const* mask, float* const* out,
                             const int* N, const int* heads, const int* nW, void* stream);
/* scatter in gather form (no atomics: thread (table row e, head h) adds the pairs of row e in a fixed order).  order int32 [N*N] =
 * the pairs i*N + j sorted by index[i*N + j] (stable), offs int32 [table_rows + 1] = start of every table row's range in it
 * (table_rows = (2ws-1)^2); both are functions of the index buffer alone (stswincl_amd/hip.py caches them per buffer).
 * nslabs > 1: dbiasT is [nslabs][heads][N][N] and the slabs are added on the way. */
int stswin_bias_scatter(const float* dbiasT, const int* order, const int* offs, float* dtable, int N, int heads, int table_rows, int nslabs,
                        void* stream);

/* ---- a6: windowed attention core (swin_512.py:117-138).  qkv [nB_*T*N][3C] = q (pre-scaled) | k | v in window
 * order; biasT [heads][N][N] and maskT [nW][N][N] are the expanded relative-position bias (:122-124) and the
 * SW-MSA mask (:126-131), both transposed to [key][query]; out [nB_*T*N][C] is the (B_, T*N, heads*d) layout of :136.
 * bwd: dqkv gets (scale*dS k | dS^T q_s | P^T dO); dbiasT [heads][N][N] += the bias gradient (per-workgroup partial slabs in
 * `scratch`, folded in a fixed order: deterministic).
 * bias_windows = 1: biasT is [heads][N][N] and maskT (or NULL) is added per window as in :126-131.
 * bias_windows = nW: biasT is [nW][heads][N][N] = bias + mask already summed by the caller, maskT must be NULL
 * (one table read per score instead of two).
 * bias_windows = U with bias_index (int [nW], values < U): biasT is [U][heads][N][N] and window w uses slot bias_index[w] - the
 * SW-MSA mask has only 4 distinct window patterns (interior, last column, last row, corner), so the 64-window table of
 * stage 1 (64 MB) shrinks to 4 MB and stays in L2. */
int stswin_win_attn_fwd(int dtype, const void* qkv, long ld, void* out, long ldo, const float* biasT, const float* maskT,
                        int nB_, int nW, int T_frames, int ws, int heads, int C, int bias_windows,
                        const int* bias_index, void* stream);
/* QKV-fused forward (swin_512.py:115-141 in one kernel; bf16, T * ws * ws = 128 tokens per window, head dim 128: the stage-1 shape):
 * out = attention(gather(x, rmap) . qkv.weight^T + qkv.bias) per (window, head), where the projection, the q scaling, the bias /
 * mask table and the softmax never leave the CU.  x [.][C] token rows, rmap int [nB_ * 128] = token row of every window row (-1:
 * zero row; NULL: identity), w = qkv.weight [3C][C] (bf16), bqkv fp32 [3C] or NULL, biasT as in stswin_win_attn_fwd with
 * bias_windows / bias_index (the pre-summed bias + mask table; no separate maskT).  qkv_out (optional, [nB_ * 128][3C]) receives
 * q * scale | k | v for stswin_win_attn_bwd; NULL in no-grad passes, which then never write q, k, v to memory.
 * x_rows = token rows of x (every rmap value is < x_rows; 0: nB_ * 128).  The kernel addresses x with 32-bit byte offsets:
 * x_rows * ldx * 2 > 0xFFFF0000 returns -1208 and launches nothing (the caller runs stswin_gemm_nt + stswin_win_attn_fwd). */
int stswin_win_attn_qkv_fwd(const void* x, long ldx, long x_rows, const int* rmap, const void* w, long ldw, const float* bqkv, void* qkv_out,
                            long ldq, void* out, long ldo, const float* biasT, int nB_, int nW, int T_frames, int ws, int heads, int C,
                            float scale, int bias_windows, const int* bias_index, void* stream);
/* BASELINE.json configs[4] "fp8 MFMA attention": the forward above with q, k, v and the probabilities quantised to OCP e4m3 in
 * registers (per (window, head) amax scales, P x 128) and both products on v_mfma_f32_32x32x16_fp8_fp8; qkv / out stay bf16 in
 * memory (same arguments, dtype fixed to bf16 storage).  A numerics mode (the non-scaled fp8 MFMA has the bf16 rate on gfx950);
 * the backward is stswin_win_attn_bwd on the unquantised qkv (straight-through). */
int stswin_win_attn_fwd_fp8(const void* qkv, long ld, void* out, long ldo, const float* biasT, const float* maskT, int nB_, int nW,
                            int T_frames, int ws, int heads, int C, int bias_windows, const int* bias_index, void* stream);
int stswin_win_attn_bwd(int dtype, const void* qkv, long ld, const void* dout, long lddo, void* dqkv, long lddq,
                        const float* biasT, const float* maskT, float* dbiasT,
                        float* dqkv_q_colsum /* optional fp32 [C]: += column sums of the dq third (q bias gradient).
                           The other two thirds need no pass over dqkv: sum_rows dk = 0 exactly (rows of dS sum to
                           zero) and sum_rows dv = column sums of dout (softmax rows sum to one) */,
                        int nB_, int nW, int T_frames, int ws,
                        int heads, int C, float scale, int bias_windows, const int* bias_index,
                        float* scratch /* >= stswin_win_attn_bwd_scratch(nB_, ws, heads, C) floats */, long scratch_floats, void* stream);
long stswin_win_attn_bwd_scratch(int nB_, int ws, int heads, int C);

/* ---- decode head on NHWC token matrices [M = frames*H*W][C]  (ASPP.py:33-52, base18.py:60-106) ---------------
 * Grouped BatchNorm2d: rows are `groups` equal groups with separate batch statistics (1 for the head; the number of
 * frames when the per-frame ResNet calls of base18.py:86-89 are batched).  colstats accumulates pivot-shifted sums
 * (sumsq may be NULL: plain grouped column sums = adaptive_avg_pool numerator, ASPP.py:43); bn_finalize turns them
 * into mean / rstd and applies nn.BatchNorm2d's running-stat update group by group; bn_apply fuses affine +
 * residual + ReLU (resnet.py:42-51); bn_bwd = the two-pass backward (s1/s2 fp32 [groups][C], zeroed by the caller).
 * unit_rows = 0: the groups are contiguous row blocks.  unit_rows > 0: group g owns the units g, g + groups, g + 2 groups, ...
 * of unit_rows rows each - frame t of every clip when the 4-frame clips are stored clip-major, so that the per-frame
 * statistics of base18.py:86-89 need no frame-major copy of the batch. */
int stswin_colstats(int dtype, const void* x, long ldx, float* sum /* += */, float* sumsq /* += */, int M, int C, int groups, int unit_rows,
                    float* scratch /* >= stswin_colstats_scratch(...) floats */, void* stream);
long stswin_colstats_scratch(int dtype, int M, int C, int groups, int unit_rows);
/* sum / sumsq [groups][N] of the statistic groups from the two-plane table a STSWIN_GF_CS_SQ stswin_gemm_nt wrote (same M, N; groups
 * of whole 256-row tiles: contiguous, or interleaved units of unit_rows rows).  Then stswin_bn_finalize with x = NULL (raw sums, no
 * pivot) replaces stswin_colstats: nn.BatchNorm2d batch statistics (resnet.py:42-51, ASPP.py:37-50) without a pass over the tensor. */
int stswin_cs_group_reduce(const float* table, int M, int N, int groups, int unit_rows, float* sum, float* sumsq, void* stream);

/* BatchNorm(train) statistics from a gemm_nt STSWIN_GF_CS_SQ table in one launch: mean / rstd [groups][N] and the running
 * statistic updates applied group by group in order (the sequential per-frame BatchNorm calls of seg18/net/Ours/base18.py:86-89;
 * torch.nn.BatchNorm2d semantics: biased variance to normalise, unbiased into running_var).  Same group geometry rules as
 * stswin_cs_group_reduce; groups <= 32.  running_* may be NULL. */
int stswin_bn_table_finalize(const float* table, int M, int N, int groups, int unit_rows, float* mean, float* rstd,
                             float* running_mean, float* running_var, float eps, float momentum, void* stream);
int stswin_bn_finalize(int dtype, const void* x, long ldx, const float* sum, const float* sumsq, float* mean, float* rstd,
                       float* running_mean, float* running_var, int M, int C, int groups, float eps, float momentum,
                       int unit_rows, void* stream);
int stswin_bn_apply(int dtype, const void* x, long ldx, const float* mean, const float* rstd, const float* gamma,
                    const float* beta, const void* resid, long ldr, void* y, long ldy, int M, int C, int groups, int relu,
                    int unit_rows, void* stream);
int stswin_bn_bwd(int dtype, const void* dy, long lddy, const void* x, long ldx,
                  const void* y /* stored output (ReLU mask); NULL with relu: the mask is recomputed from x, needs beta */,
                  long ldy, const float* mean, const float* rstd, const float* gamma, const float* beta /* may be NULL if y is given */,
                  float* s1, float* s2, void* dx, long lddx, void* dresid, long lddr,
                  int M, int C, int groups, int relu, int training,
                  int phase /* 0 both passes, 1 reduce only, 2 dx only: SyncBatchNorm all-reduces s1/s2 in between */,
                  long rows_total /* rows per group over all ranks (0 = local) */, int unit_rows,
                  float* group_sums /* optional fp32 [2][C], written by the dx pass: s1 | s2 summed over the groups = the
                                       bias | weight gradients of the BatchNorm (ASPP.py:37-50 etc.: autograd of nn.BatchNorm2d) */,
                  float* scratch /* phases 0 / 1: >= stswin_bn_bwd_scratch(...) floats (per-chunk partial sums, folded into s1 / s2) */,
                  void* stream);
long stswin_bn_bwd_scratch(int dtype, int M, int C, int groups, int unit_rows);
/* BatchNorm + ReLU + nn.MaxPool2d(3, 2, 1) in one pass (torchvision resnet18 conv1 -> bn1 -> relu -> maxpool, resnet.py:98-102):
 * x [frames*H*W][C] = the BatchNorm's input, out [frames*Hp*Wp][C] (Hp = (H-1)/2 + 1), arg (uint8, same shape) = winning tap per
 * value (first maximum in (ky, kx) scan order).  Candidates are stswin_bn_apply's values rounded to the compute dtype, so out and
 * arg equal those of stswin_bn_apply + stswin_maxpool3x3s2 (whose backward form takes arg).  Statistic groups as in stswin_bn_apply
 * (whole frames per group). */
int stswin_bn_relu_pool(int dtype, const void* x, long ldx, const float* mean, const float* rstd, const float* gamma, const float* beta,
                        void* out, long ldo, unsigned char* arg, int frames, int H, int W, int C, int groups, int unit_rows, void* stream);
/* out[r][c] (+)= v[r / (M/groups)][c] * scale : image-pool broadcast (ASPP.py:46) and avg-pool backward */
int stswin_rows_broadcast(int dtype, const float* v, void* out, long ldo, int M, int C, int groups, float scale,
                          int accumulate, void* stream);
/* bilinear, align_corners=False (base18.py:102-103): forward in[F][h][w][C] -> out[F][H][W][C]; backward: in = d(out),
 * out = d(in) (gather form, no atomics) */
int stswin_bilinear(int dtype, const void* in, long ldi, void* out, long ldo, int frames, int h, int w, int H, int W, int C,
                    int backward, void* stream);
/* final interpolate of base18.py:106: tokens [F][h][w][nc] <-> NCHW logits [F][nc][H][W] */
int stswin_logits_upsample(int dtype, const void* tokens, long ldt, void* nchw, int frames, int h, int w, int H, int W,
                           int nc, int backward, void* stream);

/* ---- a15: OHEM cross entropy (seg18/utils/losses.py:32-40).  ce_fwd: per-pixel CE (ignore_index -> 0) and
 * stats (fp32 [4], zeroed by the caller, 8-byte aligned): [0] = #(loss > thresh) (an exact integer count), [1] = #pixels whose label
 * is neither ignore_index nor in [0, nc) (their loss is NaN and the logits are not read at such a label; ohem_select then returns
 * NaN), [2..3] = one unsigned 64-bit sum of the counted losses in 2^-32 fixed point (integer atomics: associative, so the value is
 * reproducible).  ce_bwd: dlogits = gscale[0] * w * (softmax - onehot), w = sel[1] for pixels with loss > sel[0], sel[3] for loss
 * == sel[0], else 0 (and 0 at ignore_index or an out-of-range label); sel/gscale live on the device, so no host sync is needed. */
int stswin_ce_fwd(int dtype, const void* logits, const long* labels, float* loss, float* stats, int frames, long HW, int nc,
                  int ignore_index, float thresh, void* stream);
/* The selection of losses.py:35-39 without the sort: value[0] = OHEM loss, sel[4] = (cut, weight above the cut, top-n_min branch
 * taken, weight at the cut) for ce_bwd.  stats = output of ce_fwd; if stats[0] = #(loss > thresh) > n_min the threshold branch is
 * taken (cut = thresh, 1/count above it, 0 at it), otherwise the mean of the n_min largest losses is computed by an exact 3-level
 * radix select (counts + sums per bin): cut = the k-th largest loss, 1/n_min above it, and the t losses tied AT the cut share the
 * k_rem places left, k_rem / (t * n_min) each (the reference's gradient averaged over the orders of the ties).  value[0] is NaN when
 * stats[1] != 0 (labels outside [0, nc)).  work: caller-owned scratch
 * of >= STSWIN_OHEM_WORK_BYTES bytes (zeroed by the call). */
#define STSWIN_OHEM_WORK_BYTES (3 * 2048 * 12 + 48)
int stswin_ohem_select(const float* loss, long n, long n_min, float thresh, const float* stats, void* work, long work_bytes,
                       float* value, float* sel, void* stream);
int stswin_ce_bwd(int dtype, const void* logits, const long* labels, const float* loss, const float* sel,
                  const float* gscale, void* dlogits, int frames, long HW, int nc, int ignore_index, void* stream);

/* ---- a16/a17: label-guided pixel-contrastive similarity (pixcontrast_18/contrast/models/PixPro_swin_v5.py:71-129).
 * Q [N][HW][C] query embeddings, K5[j] [N][HW][C] the five key maps (k, adj1, adj2, adj3, neg3), lq / lk5[j] int32
 * labels [N][HW].  Writes pos[n][i][j] = sum_p (q_i . k_jp) [lq_i == lk_jp] and all[n][i][j] = sum_p q_i . k_jp
 * (fp32 [N][HW][5]); the HW x HW logits / posMask / negMask tensors of :82-113 are never materialised. */
int stswin_contrast_fwd(int dtype, const void* Q, long ldq, const void* const* K5, long ldk, const int* lq,
                        const int* const* lk5, float* pos, float* all, int N, int HW, int C, void* stream);

/* Bank mode of the same loss: every query pixel against a bank of key embeddings, ONE launch for both loss directions and all
 * key maps (PixPro_swin_v5.py:594-595 = two regression_loss calls, :71-129), and the inter-video bank that the reference
 * sketches in its unused dist_collect (pixcontrast_18/contrast/util.py:47-58).
 *   Q [M][C] + lq[M]: the M query rows are q_sets (1 or 2: the loss directions) equal sets of nblk = M / (q_sets q_block) blocks of
 *     q_block rows (a block = one sample's HW pixels in the reference's per-sample mode; q_block = M / q_sets: one block, every
 *     query sees the whole segment);
 *   bank [maps][seg][C] + lb[maps][seg]: query set s uses map gmap[s*groups + g] as its group g; a query of block b sees rows
 *     [b bank_block, (b+1) bank_block) of that map (bank_block = seg / nblk, or = seg when nblk = 1).
 * Writes pos[m][g] = sum_p S[m][p] [lq[m] == lb[p]], all[m][g] = sum_p S[m][p] over the visible rows of group g (fp32 [M][groups]) and,
 * if not NULL, rowmax[m] / lse[m] = max / log-sum-exp of inv_tau * S[m][p] over the visible rows of ALL groups (the InfoNCE
 * denominator; monitoring and hard-negative statistics - the reference loss itself is linear in S).  C: bf16 64, 128, 192 or 256;
 * fp32 32, 64, 128 or 256 (the kernel is instantiated per C / 32 in {1, 2, 4, 8}: fp32 96, 160, 192 and 224 are refused with -1516,
 * like every refusal before anything is launched).  Q rows need 16-byte alignment (ldq a multiple of 8 (bf16) / 4 (fp32) elements),
 * bank rows likewise.  workspace: caller-owned fp32 scratch, >= 4 M groups floats (more lets the launcher split long bank segments
 * over workgroups; the partials are combined in a fixed order, so results are deterministic).
 *
 * LABELS must lie in [0, ncls) (ncls <= 63 for stswin_contrast_class_sums, <= 64 for stswin_label_counts).  The reference's F.one_hot
 * raises outside that range (PixPro_swin_v5.py:54), so it defines nothing there, and the kernels of this section DIFFER there:
 *   - the forward (stswin_contrast_fwd, stswin_contrast_bank_fwd / _unit) compares the raw int32 labels: -3 matches -3 and nothing else;
 *   - stswin_label_counts clamps query and bank labels to [0, ncls - 1] before counting: -3 counts as class 0, ncls + 5 as ncls - 1;
 *   - stswin_contrast_class_sums adds a bank row with such a label to the total (slot ncls) only, and stswin_contrast_bank_dq gives a
 *     query with such a label an all-zero class row.
 * For such labels the gradient of class_sums + bank_dq is therefore NOT the derivative of the forward's sums, and cnt is not the
 * size of the forward's positive set.  Callers keep labels in range. */
int stswin_contrast_bank_fwd(int dtype, const void* Q, long ldq, const int* lq, int M, int C, int q_sets, int q_block,
                             const void* bank, long ldb, const int* lb, int maps, int seg, int bank_block, int groups,
                             const int* gmap /* host memory, [q_sets][groups] */, float inv_tau, float* pos, float* all,
                             float* rowmax, float* lse, float* workspace, long workspace_floats, void* stream);
/* The same for L2-NORMALISED query and bank rows (the embeddings ConsistencyLoss feeds it: F.normalize, PixPro_swin_v5.py:369-557):
 * |S| <= 1, so rowmax / lse are formed with inv_tau as a FIXED reference point of the sum of exponentials - one fma + one exponential
 * per score instead of a running maximum with rescaling (same values to fp32 rounding; the caller guarantees the norms). */
int stswin_contrast_bank_fwd_unit(int dtype, const void* Q, long ldq, const int* lq, int M, int C, int q_sets, int q_block,
                             const void* bank, long ldb, const int* lb, int maps, int seg, int bank_block, int groups,
                             const int* gmap /* host memory, [q_sets][groups] */, float inv_tau, float* pos, float* all,
                             float* rowmax, float* lse, float* workspace, long workspace_floats, void* stream);
/* Backward to the queries (keys are no-grad, PixPro_swin_v5.py:366): the masked sums are linear in the scores, so
 * dq[m] = sum_g dpos[m][g] Kcls[map(g)][blk][lq[m]] + dneg[m][g] (Ktot[map(g)][blk] - Kcls[..][lq[m]]), where dpos / dneg are the
 * gradients of pos and of neg = all - pos.  class_sums writes ksum [maps][seg / bank_block][ncls + 1][C] fp32 (slot ncls = all
 * rows; zeroed by the call; 1 <= ncls <= 63, C % 4 == 0, C <= 512; labels outside [0, ncls) only count in the total); bank_dq
 * combines them per query row into dq fp32 [M][C] (seg / bank_block = the number of query blocks or 1, else -1532).  cnt[m][g] (fp32) = number of visible rows of group g with label lq[m]: where it equals bank_block the negative
 * set is empty and its term is skipped, so the gradient is exactly zero like the reference's masked products (:103-113). */
int stswin_contrast_class_sums(int dtype, const void* bank, long ldb, const int* lb, int maps, int seg, int bank_block, int C,
                               int ncls, float* ksum, float* scratch /* >= stswin_contrast_class_sums_scratch(...) floats */, void* stream);
long stswin_contrast_class_sums_scratch(int maps, int seg, int bank_block, int C, int ncls);
int stswin_contrast_bank_dq(const float* dpos, const float* dneg, const float* cnt, const int* lq, const float* ksum, float* dq,
                            long lddq, int M, int C, int q_sets, int q_block, int seg, int bank_block, int ncls, int groups, const int* gmap,
                            void* stream);

/* ---- the glue of the contrastive step (round 5; pixcontrast_18/contrast/models/PixPro_swin_v5.py): what the reference does in ~125
 * elementwise torch launches per step.
 * stswin_rownorm_scatter: Y[(view, sample, pixel)] = X[row] / max(||X[row]||_2, 1e-12), fp32 arithmetic, compute-dtype result
 *   (F.normalize(proj.float(), dim=1) of PixPro._embed, :369-557) with the batched views de-interleaved: X rows are clip-major
 *   ((sample * views + view) * HW + pixel), Y is the view-major [views][samples * HW][C] matrix the pair loss reads (its key bank /
 *   query matrix: no NCHW permute, slice, stack or cat in between).  inv (optional) keeps 1 / norm per row for the backward:
 *   dX = inv (dY - y (y . dY)).  C % 64 == 0, C <= 1024, R == views * samples * HW.
 * stswin_labels_resize: `maps` (<= 8) float label maps [N][1][Hs][Ws] -> int32 lb[maps][N * h * w], nearest neighbour with ATen's index
 *   rule (F.interpolate(mode='nearest') + .to(int32), ConsistencyLoss.forward :590-593).
 * stswin_label_counts: cnt[m][g] = number of rows of bank block blk(m) of map gmap[set(m)][g] whose label equals lq[m] (labels clamped
 *   to [0, ncls - 1]; 1 <= ncls <= 64): the row sums of posMask (:48-57, :116-118) from per-block class histograms (hist: int scratch
 *   [maps][seg / bank_block][ncls]).  Block geometry as stswin_contrast_bank_fwd: M % (q_sets q_block) == 0 and seg / bank_block equal
 *   to the number of query blocks M / (q_sets q_block) or to 1, else -1543 before anything is launched.
 * stswin_pair_loss / _bwd: loss = sum over the query sets of mean(-log(e^P / (e^P + e^N) + 1e-6)), P = sum_g pos_g / (sum_g cnt_g + 1e-6),
 *   N = sum_g (all_g - pos_g) / (visible - cnt_g + 1e-6) (:119-129); one workgroup, fixed-order sums (deterministic); the backward gives
 *   d loss / d pos and d loss / d (all - pos). */
int stswin_rownorm_scatter(int dtype, const void* X, long ldx, void* Y, long ldy, float* inv, int R, int C, int views, int HW, int samples,
                           void* stream);
int stswin_rownorm_scatter_bwd(int dtype, const void* X, long ldx, const float* inv, const float* dY, long lddy, void* dX, long lddx, int R,
                               int C, int views, int HW, int samples, void* stream);
int stswin_labels_resize(const float* const* masks, int maps, int N, int Hs, int Ws, int h, int w, int* lb, void* stream);
int stswin_label_counts(const int* lq, const int* lb, int M, int maps, int seg, int q_sets, int q_block, int bank_block, int ncls, int groups,
                        const int* gmap, int* hist, float* cnt, void* stream);
int stswin_pair_loss(const float* pos, const float* all, const float* cnt, int M, int groups, int q_sets, int visible, float* loss,
                     void* stream);
int stswin_pair_loss_bwd(const float* pos, const float* all, const float* cnt, const float* dloss, int M, int groups, int q_sets, int visible,
                         float* dpos, float* dneg, void* stream);

/* ---- f4: inference post-processing (seg18/test.py:153-158 + utils/EndoMetric.py): labels[f][y][x] = argmax_c of the
 * bilinear (align_corners = True) resize of NCHW logits [F][nc][h][w] (nc <= 64) to (H, W); the first maximum wins.  With gt (int64
 * [F][H][W]) also counts[f][0|1|2][c] += |gt == c|, |pred == c|, |gt == c and pred == c| for c < nc (int32, zeroed by the caller).  gt
 * is compared as int64: a value outside 0 .. nc-1, 2^32 + 3 included, is no class, as for the two entries that count below.
 * Errors (nothing is launched): -1406 nc outside 1 .. 64; frames, h, w, H or W <= 0; logits or labels NULL; gt without counts. */
int stswin_upsample_argmax(int dtype, const void* logits, unsigned char* labels, const long* gt, int* counts, int frames,
                           int nc, int h, int w, int H, int W, void* stream);
/* ---- CaDIS evaluation (segcata/cata_test.py:115-170 + utils/cata_metrics.py ConfusionMatrix): labels[f][y][x] = argmax_c of the
 * bilinear resize of NCHW logits [F][nc][h][w] (nc <= 64) to (H, W), align_corners = 1 as stswin_upsample_argmax, 0 as ATen
 * (cata_test.py:129: src = max((in / out) (dst + 0.5) - 0.5, 0)); first maximum wins.  labels may be NULL (not written).  With gt
 * (int64 [F][H][W]) and cm (uint64 [ncm][ncm], ncm <= 64) every pixel with 0 <= gt < ncm and 0 <= label < ncm adds 1 to
 * cm[gt][label] (rows gt, columns prediction, as the reference's `num_classes * gt + pred`).  The matrix is accumulated, never
 * cleared: the caller zeroes it once per evaluation.  gt is compared as int64.  Integer atomics only (exact, independent of order).
 * Errors (nothing is launched): -1406 nc outside 1 .. 64, or frames, h, w, H or W <= 0; -1407 logits NULL; -1408 gt without cm, cm
 * without gt, or (with both) ncm outside 1 .. 64; -1409 neither cm nor labels. */
int stswin_upsample_argmax_cm(int dtype, const void* logits, unsigned char* labels, const long* gt, unsigned long long* cm, int ncm,
                              int align_corners, int frames, int nc, int h, int w, int H, int W, void* stream);
/* ---- colour overlay of a label map (stswincl_amd/utils/visualize.py, VideoSegmenter(out="overlay")): labels uint8 [n][H][W],
 * frames uint8 [n][H][W][3] (HWC RGB) or NULL (every source byte 0), table uint8 [256][4] = (r, g, b, a) per label value, out uint8
 * [n][H][W][3].  Per pixel and channel, with s the frame byte and (c, a) the table entry of the pixel's label:
 *     out = (a c + (255 - a) s + 127) / 255        (integer division: a = 255 gives c, a = 0 gives s, both exactly)
 * edge_alpha = -1: no outlines; 0 .. 255: a pixel whose label differs from that of its left, right, upper or lower neighbour inside
 * the same frame (no wrap to the next row, no look into the next frame) uses a = edge_alpha with its own colour.  out may alias
 * frames (a thread reads only the frame bytes of the pixels it writes), not labels.  Any pointer alignment, any W: pointers that are
 * all 8-byte aligned take the body with 8 pixels per thread, others the byte body.  Integer arithmetic only.
 * Errors: -1415 n, H or W <= 0; -1416 labels, table or out NULL; -1417 edge_alpha outside -1 .. 255. */
int stswin_labels_overlay(const unsigned char* labels, const unsigned char* frames, const unsigned char* table, unsigned char* out,
                          int n, int H, int W, int edge_alpha, void* stream);
/* ---- ground truth as the files hold it -> class indices (stswincl_amd/utils/groundtruth.py, VideoSegmenter(gt_table=...)): in uint8
 * [n][H][W][ch], out [n][H][W] of out_bytes = 1 (uint8, what stswin_labels_overlay reads) or 8 (int64, what stswin_upsample_argmax
 * and stswin_upsample_argmax_cm read as gt).
 *   ch = 3 | 4, colour-coded (seg18/dataset/Endovis2018_new.py:130-136): table uint8 [ncolours][4] = (r, g, b, label), 1 <= ncolours
 *     <= 256.  A pixel takes the label of the LAST row whose (r, g, b) equals its first three channels exactly (the fourth channel
 *     is not looked at); a pixel that equals no row gets 0 and, when `unmatched` (int32 [n], may be NULL) is given, adds 1 to
 *     unmatched[its frame].  unmatched is accumulated, never cleared: the caller zeroes it once per evaluation.
 *   ch = 1, id-coded (segcata/dataset/CATA_new_512.py:97, 237): table uint8 [256], out = table[u]; ncolours is range-checked and
 *     otherwise unused, unmatched is left alone.
 * One launch, no scratch buffer, no synchronisation (graph-capturable).  Any pointer alignment, any W: `in` 16-byte (ch = 4) or
 * 4-byte (ch = 1, 3) aligned together with `out` 4-byte (uint8) or 16-byte (int64) aligned takes the body with 4 pixels per thread,
 * anything else the byte body.  Integer atomics only (exact, independent of order).
 * Errors: -1418 n, H or W <= 0; -1419 in, table or out NULL; -1420 ch not 1, 3 or 4; -1421 ncolours outside 1 .. 256; -1422 out_bytes
 * not 1 or 8; -1423 out overlaps in. */
int stswin_gt_decode(const unsigned char* in, const unsigned char* table, void* out, int* unmatched, int n, int H, int W, int ch,
                     int ncolours, int out_bytes, void* stream);
/* ---- per-frame instrument report (stswincl_amd/utils/instruments.py, VideoSegmenter(report=...)): labels uint8 [n][H][W], out int64
 * [n][nc][10].  Row out[f][c][0..9], taken over the pixels (y, x) of frame f whose label equals c:
 *     0: count      1, 2: sum x, sum y      3, 4, 5: sum x^2, sum xy, sum y^2
 *     6, 7: max(W - x), max(H - y)          8, 9: max(x + 1), max(y + 1)
 * The extent is four maxima so that an all-zero row means "class absent"; the half-open box of a present class is
 * [W - out[6], out[8]) x [H - out[7], out[9]).  Pixels with label >= nc are counted nowhere.  out is accumulated, never cleared (sums
 * add, extents take the maximum): the caller zeroes it, and may pool several calls in one buffer.  1 <= nc <= 64 and 1 <= H, W <=
 * 16384, so every sum fits an int64 (sum x^2 <= 2^28 2^28).  Integer atomics only (exact, independent of order: bit-reproducible).
 * One launch, no scratch buffer, no synchronisation (graph-capturable).  Any pointer alignment, any W: labels 16-byte aligned with
 * W % 16 == 0 takes the body with 16 pixels of one row per thread from one 16-byte load, anything else the byte body.
 * Errors: -1545 n, H or W <= 0, or H or W > 16384 (or more workgroups than a grid holds); -1546 labels or out NULL; -1547 nc outside
 * 1 .. 64.  (-1544 is stswin_pair_loss's.) */
int stswin_label_moments(const unsigned char* labels /*[n][H][W]*/, long long* out /*[n][nc][10]*/, int n, int H, int W, int nc,
                         void* stream);
/* ---- connected instances of a label map (stswincl_amd/utils/instruments.py label_components, VideoSegmenter(instances=K)): labels
 * uint8 [n][H][W] -> components int32 [n][H][W], rows int64 [n][K][12], total int32 [n].  A component is a maximal set of pixels of
 * one frame with the same label c < nc, bit c of `skip` clear, joined under connectivity 4 or 8; a frame's components of all classes
 * are numbered 0, 1, 2, ... by their first pixel in raster order (the smallest y W + x they hold).
 *   components  every pixel's ordinal, not bounded by K; -1 for a skipped label or a label >= nc
 *   total[f]    the number of components of frame f, not bounded by K
 *   rows[f][i]  for i < min(total[f], K):   0: class   1: first = y W + x of the first pixel   2 .. 11: the ten integers of
 *               stswin_label_moments over the component's pixels (count, sum x, sum y, sum x^2, sum xy, sum y^2, max(W - x),
 *               max(H - y), max(x + 1), max(y + 1)); all zero from total[f] on.  With total[f] > K the rows kept are the first K in
 *               that order, whatever the order of execution; components and total are complete even then.
 * All three outputs are written in full by the call (rows is cleared by a fill kernel on the stream, no memset node).  workspace:
 * caller-owned, 4-byte aligned, >= stswin_label_components_scratch(n, H, W) bytes (an int32 parent map and the counts of the
 * numbering pass); nothing in it needs clearing and nothing survives the call.  Seven launches (six when the map is one tile), no
 * synchronisation, no allocation (graph-capturable); no kernel waits on another workgroup.  Integer atomics only (exact, independent
 * of order: bit-reproducible).  Any pointer alignment of labels, any W; 1 <= H, W <= 16384.  The buffers must not overlap (the host
 * wrapper checks).
 * Errors, before anything is launched: -1830 n, H or W <= 0, or H or W > 16384 (or more workgroups than a grid holds; also what
 * stswin_label_components_scratch returns for such a shape); -1831 labels, components, rows, total or workspace NULL; -1832 nc
 * outside 1 .. 64; -1833 connectivity not 4 or 8; -1834 K outside 1 .. 1024; -1835 workspace_bytes too small or workspace not 4-byte
 * aligned. */
long stswin_label_components_scratch(int n, int H, int W);
int stswin_label_components(const unsigned char* labels /*[n][H][W]*/, int* components /*[n][H][W]*/, long long* rows /*[n][K][12]*/,
                            int* total /*[n]*/, int n, int H, int W, int nc, int connectivity, long skip, int K, void* workspace,
                            long workspace_bytes, void* stream);
/* the geometry of stswin_label_components (the tests place their shapes around it): which = 0, 1: height and width in pixels of the
 * tile a workgroup labels in LDS (16, 64), 2: the pixels of a raster chunk of the numbering pass (2048); anything else: -1. */
int stswin_label_components_geometry(int which);
/* ---- instances followed from frame to frame (stswincl_amd/utils/instruments.py InstanceTracker, VideoSegmenter(tracks=True)): the
 * components, rows [K][12] and total [1] of ONE frame of stswin_label_components, frame after frame in frame order -> ids int32 [K],
 * started int32 [1].  Instance j takes part if j < min(total, K) and rows[j][2] >= min_area.  ov[i][j] = the pixels that carry ordinal
 * i in the previous call's map and j in this one (-1 and ordinals >= K count nowhere), u = area[i] + area[j] - ov.  A previous
 * participant i and a current one j are a candidate iff ov > 0, their classes are equal (same_class = 1; 0 drops the condition) and
 * 1000 ov >= min_iou u (min_iou in thousandths, 0 .. 1000; int64).  (i, j) is preferred to (i', j') iff ov u' > ov' u (int64
 * products), then smaller i, then smaller j.  Repeatedly the most preferred candidate whose i and j are both unmatched is matched and
 * ids[j] = the id of i; the participants left over take next, next + 1, ... in ascending j; every other entry of ids is -1; started =
 * next after the call.  Bit for bit InstanceTracker.update, whatever the order of execution (integer atomics only).
 * state: caller-owned, 16-byte aligned, >= stswin_track_state_bytes(H, W, K) bytes, int32 words:
 *   [0] next id   [1] listed pairs   [2], [3] unused   cls[K], area[K], id[K] of the previous call's instances (cls -1: takes no part)
 *   ov[K][K]   list[K K]: the pairs i << 10 | j with ov != 0   then, 16-byte aligned, the previous map [H W], padded with -1 to a
 *   multiple of four pixels.
 * stswin_track_reset (one fill kernel, no memset node) starts a sequence: next = 0, no previous instances, a previous map of -1, ov
 * and the list cleared; a state must be reset once before its first use.  stswin_track_instances is two launches: the overlap pass
 * reads both maps once (16-byte loads; 4-byte loads of a `components` that is only 4-byte aligned), writes the current map over the
 * previous one in the same pass and counts the pairs on chip, one global atomic per distinct pair and workgroup; one workgroup then
 * matches, writes ids, started and the new state and clears what the overlap pass counted.  No allocation, no synchronisation,
 * `total` is read on the device only (graph-capturable); no kernel waits on another workgroup.  The buffers must not overlap (the host
 * wrapper checks).
 * Errors, before anything is launched: -1840 H or W <= 0 or > 16384; -1841 K outside 1 .. 1024 (stswin_track_state_bytes returns
 * these two as well); -1842 a NULL pointer; -1843 state_bytes too small or state not 16-byte aligned; -1844 components, total, ids or
 * started not 4-byte aligned, or rows not 8-byte aligned; -1845 min_iou outside 0 .. 1000, same_class not 0 or 1, or min_area < 1. */
long stswin_track_state_bytes(int H, int W, int K);
int stswin_track_reset(void* state, long state_bytes, int H, int W, int K, void* stream);
int stswin_track_instances(const int* components /*[H][W]*/, const long long* rows /*[K][12]*/, const int* total /*[1]*/, void* state,
                           long state_bytes, int H, int W, int K, int min_iou, int same_class, int min_area, int* ids /*[K]*/,
                           int* started /*[1]*/, void* stream);
/* ---- the tracker with a memory (stswincl_amd/utils/instruments.py MemoryTracker, VideoSegmenter(tracks=True, track_max_gap=g)): the
 * same inputs and outputs as stswin_track_instances, with a state of its own.  A track that no instance is matched to stays alive for
 * up to max_gap calls, and instances are matched against the mask the track had when it was last seen: mem[p] is the track pixel p is
 * remembered for.  Instance j takes part as above.  ov[t][j] = the pixels with mem == t that carry ordinal j in this call's map, u =
 * area[t] + area[j] - ov with area[t] the track's area at its last sighting.  (t, j) is a candidate iff ov > 0, the classes are equal
 * (same_class = 1) and 1000 ov >= min_iou u.  (t, j) is preferred to (t', j') iff ov u' > ov' u (int64 products), then the smaller
 * track id, then smaller j.  Repeatedly the most preferred candidate whose t and j are both unmatched is matched and ids[j] = t; the
 * participants left over take next, next + 1, ... in ascending j; every other entry of ids is -1; started = next after the call.  A
 * matched track takes the instance's class and area and age 0, a new track has age 0, every other live track ages by one and ends
 * when its age exceeds max_gap.  If more than K tracks live then, lost ones (age >= 1) end until K do, the largest age first, then the
 * smallest id.  A pixel of a participant j then takes ids[j]; any other pixel becomes -1 if its track ended or was matched in this
 * call and stays otherwise.  Bit for bit MemoryTracker.update, whatever the order of execution (integer atomics only); with max_gap =
 * 0 every unmatched track ends at once.
 * state: caller-owned, 16-byte aligned, >= stswin_track_memory_state_bytes(H, W, K) bytes, int32 words.  The live tracks sit in K
 * slots; which slot a track has shows in no output:
 *   [0] next id   [1] listed pairs   [2], [3] unused   cls[K] (-1: a free slot), area[K], id[K], age[K] of the slots   slot_of[K]: the
 *   slot of each ordinal of the last call (-1: took no part)   keep[K]: 1 for the slots whose remembered pixels the last call kept
 *   ov[K][K] (slot, ordinal)   list[K K]: the pairs slot << 10 | j with ov != 0   then, 16-byte aligned, the memory map [H W] of slots,
 *   padded with -1 to a multiple of four pixels.
 * stswin_track_memory_reset (one fill kernel, no memset node) starts a sequence: next = 0, every slot free, a memory map of -1, ov and
 * the list cleared; a state must be reset once before its first use.  stswin_track_memory is three launches: the overlap pass of
 * stswin_track_instances over the memory map and `components`, which writes neither; one workgroup that matches, writes ids and
 * started, ages, ends and evicts tracks, gives births the free slots, leaves slot_of and keep and clears what the overlap pass
 * counted; and a commit pass over both maps, four pixels per thread with both tables in LDS, mem = the pixel's instance takes part ?
 * slot_of[components] : (mem >= 0 and keep[mem] ? mem : -1).  No allocation, no synchronisation, `total` is read on the device only
 * (graph-capturable); no kernel waits on another workgroup.  The buffers must not overlap (the host wrapper checks).
 * Errors, before anything is launched: -1860 H or W <= 0 or > 16384; -1861 K outside 1 .. 1024 (stswin_track_memory_state_bytes
 * returns these two as well); -1862 a NULL pointer; -1863 state_bytes too small or state not 16-byte aligned; -1864 components, total,
 * ids or started not 4-byte aligned, or rows not 8-byte aligned; -1865 min_iou outside 0 .. 1000, same_class not 0 or 1, or min_area
 * < 1; -1866 max_gap outside 0 .. 1000000. */
long stswin_track_memory_state_bytes(int H, int W, int K);
int stswin_track_memory_reset(void* state, long state_bytes, int H, int W, int K, void* stream);
int stswin_track_memory(const int* components /*[H][W]*/, const long long* rows /*[K][12]*/, const int* total /*[1]*/, void* state,
                        long state_bytes, int H, int W, int K, int max_gap, int min_iou, int same_class, int min_area, int* ids /*[K]*/,
                        int* started /*[1]*/, void* stream);
/* ---- run-length masks (stswincl_amd/utils/rle.py encode, VideoSegmenter(masks=...)): a map uint8 (elem_bytes 1: a label map) or int32
 * (elem_bytes 4: the components of stswin_label_components) [n][H][W] -> runs int32 [n][cap][2], count int32 [n].  Frame f is read in
 * column-major order, v[p] = map[f][y][x] with p = x H + y (COCO's order: a run continues from the bottom of column x - 1 into the top
 * of column x).  A run starts at p = 0 and wherever v[p] != v[p - 1]; R is the number of run starts.
 *   count[f]    R, not bounded by cap
 *   runs[f][i]  for i < min(R, cap): (p_i, v[p_i]) of the i-th run start in ascending p, a uint8 value zero-extended, an int32 value
 *               as it is (-1 included); all zero from min(R, cap) on.  With R > cap the runs kept are the first cap, whatever the order
 *               of execution; count is complete even then.
 * Both outputs are written in full by the call (the tail of runs by the third launch, no memset node).  workspace: caller-owned,
 * 4-byte aligned, >= stswin_rle_encode_scratch(n, H, W) bytes (the starts per column and segment of 32 rows, int32 [n][W][S]); nothing
 * in it needs clearing and nothing survives the call.  Three launches - count per column and segment, one workgroup per frame scans,
 * the same walk again stores - no synchronisation, no allocation, no host read (graph-capturable); no kernel waits on another
 * workgroup.  No atomics: every word has one writer (bit-reproducible).  1 <= H, W <= 16384 (p < 2^28), 1 <= cap <= 1048576, any W;
 * map aligned to elem_bytes: 16-byte aligned with rows of a multiple of 16 bytes takes the body with one 16-byte load per thread and
 * row, anything else the element body.  The buffers must not overlap (the host wrapper checks).
 * Errors, before anything is launched: -1850 n, H or W <= 0, or H or W > 16384 (or more workgroups than a grid holds; also what
 * stswin_rle_encode_scratch returns for such a shape); -1851 map, runs, count or workspace NULL; -1852 elem_bytes not 1 or 4; -1853 cap
 * outside 1 .. 1048576; -1854 workspace_bytes too small or workspace not 4-byte aligned; -1855 map not aligned to elem_bytes, or runs
 * or count not 4-byte aligned. */
long stswin_rle_encode_scratch(int n, int H, int W);
int stswin_rle_encode(const void* map /*[n][H][W]*/, int elem_bytes /*1: uint8, 4: int32*/, int* runs /*[n][cap][2]*/,
                      int* count /*[n]*/, int n, int H, int W, int cap, void* workspace, long workspace_bytes, void* stream);
/* the geometry of stswin_rle_encode (the tests place their shapes around it): which = 0: rows of a segment (32), 1: columns of a
 * workgroup's band (256), 2: pixels per thread and row (16 for uint8; a thread of an int32 map takes 4); anything else: -1. */
int stswin_rle_geometry(int which);
/* ---- boundary scores (stswincl_amd/utils/boundary.py boundary_counts, VideoSegmenter(boundary=...)): gt int64 [n][H][W] and pred uint8
 * [n][H][W] -> out int32 [n][nc][2][2 + bins], what the normalised surface distance and the Hausdorff distance are made of.  For a map M
 * and a class c < nc the contour B_c(M) is the set of pixels with M == c that have a 4-neighbour with M != c, a neighbour outside the
 * image counting as different (mask & ~binary_erosion(mask)); a value outside 0 .. nc-1 belongs to no class.  Row out[f][c][d], d = 0:
 * the contour of gt measured against the one of pred, d = 1: pred against gt; d2(p) = the minimum over the pixels q of the other contour
 * of |p - q|^2, an exact integer:
 *     0: the number of pixels of the own contour          1: the maximum of d2 over them, -1 when either contour is empty
 *     2 + k, k < bins - 1: the own contour pixels whose ceil(sqrt(d2)) == k (the smallest k with k^2 >= d2)
 *     2 + bins - 1: those with ceil(sqrt(d2)) >= bins - 1           (the histogram is all zero when either contour is empty)
 * The rows of the classes whose bit of skip_mask is set are all zero.  out is written in full by the call (a fill kernel on the stream,
 * no memset node); nothing needs clearing beforehand.  workspace: caller-owned, 8-byte aligned, >= stswin_boundary_scratch(n, H, W, nc)
 * = 16 n (S W + 1) + 2 n H W (2 nc + 1) bytes with S = ceil(H / 64) (per map, segment of 64 rows and column the classes with a contour
 * pixel there, uint64 [2][n][S][W]; each map's classes, uint64 [2][n]; per map and class the column distances uint16
 * [2][n][nc][H][W]; the contour codes uint8 [2][n][H][W]);
 * nothing in it needs clearing and nothing survives the call.  Five launches whatever nc and the maps hold - fill, mark the contours,
 * classes per segment, column distances, query - no synchronisation, no allocation, no host read (graph-capturable); no kernel waits
 * on another workgroup.  Integer arithmetic and integer atomics only (add and max into out, or into the workspace): exact, independent of the order (bit-reproducible); the
 * float square root only seeds the ceiling, integer comparisons decide it.  gt 8-byte and out 4-byte aligned, pred at any address, any
 * W; 1 <= H, W <= 16384 (d2 < 2^30), 1 <= nc <= 64, 2 <= bins <= 256.  The buffers must not overlap (the host wrapper checks).
 * Errors, before anything is launched: -1870 n, H or W <= 0, or H or W > 16384 (or more workgroups than a grid holds; also what
 * stswin_boundary_scratch returns for such a shape); -1871 gt, pred, out or workspace NULL; -1872 nc outside 1 .. 64 (from
 * stswin_boundary_scratch too); -1873 bins outside 2 .. 256; -1874 workspace_bytes too small or workspace not 8-byte aligned; -1875 gt
 * not 8-byte or out not 4-byte aligned. */
long stswin_boundary_scratch(int n, int H, int W, int nc);
int stswin_boundary_counts(const long long* gt /*[n][H][W]*/, const unsigned char* pred /*[n][H][W]*/, int* out /*[n][nc][2][2+bins]*/,
                           int n, int H, int W, int nc, int bins, long skip_mask, void* workspace, long workspace_bytes, void* stream);
/* the geometry of stswin_boundary_counts (the tests place their shapes around it): which = 0, 1: height and width in pixels of the tile
 * a workgroup of the query pass owns (16, 64), 2: the columns of a workgroup of the column pass (64), 3: the rows of a segment of the
 * column pass (64); anything else: -1.  The query pass
 * gathers in LDS while nc (2 + bins) <= 8192 words and adds to out directly above that. */
int stswin_boundary_geometry(int which);
/* ---- confidence of the labels (stswincl_amd/utils/confidence.py, VideoSegmenter(confidence=...)): the softmax probability that
 * seg18/test.py:153-158 computes between its resize and its argmax, for the label each pixel got.  logits NCHW [F][nc][h][w] (dtype 0
 * bf16, 1 fp32), labels uint8 [F][H][W] (of stswin_upsample_argmax / stswin_upsample_argmax_cm, or any other), conf uint8 [F][H][W].
 * v_c is the bilinear value of class c at the output pixel, by the fp32 coordinate and value expressions of those two label launches
 * (align_corners = 1: src = dst (in - 1) / (out - 1); 0: src = max((in / out) (dst + 0.5) - 0.5, 0)), so for a label they made
 * v_label is the maximum to the bit.  With m = max_c v_c and l the pixel's label
 *     p = exp(v_l - m) / sum_c exp(v_c - m)          conf = min(255, floor(255 p + 0.5)),   conf = 0 for l >= nc
 * in fp32 with expf, the maximum and the sum taken online in one pass over the classes.  One launch, no scratch buffer, no atomics, no
 * synchronisation (graph-capturable); the result depends on nothing but the inputs.  A thread takes four pixels of one row (they share
 * the row's weights): labels and conf 4-byte aligned with W % 4 == 0 takes the body with one 4-byte load and store, anything else
 * the byte body.  1 <= nc <= 64, h w < 2^31.  conf must not overlap labels or logits (the host wrapper checks).
 * Errors, before anything is launched: -1880 frames, h, w, H or W <= 0, h w >= 2^31 (or more workgroups than a grid holds); -1881 nc
 * outside 1 .. 64; -1882 logits, labels or conf NULL; -1883 dtype not 0 or 1. */
int stswin_upsample_confidence(int dtype, const void* logits, const unsigned char* labels, unsigned char* conf, int align_corners,
                               int frames, int nc, int h, int w, int H, int W, void* stream);
/* sums of a confidence map over a label map or a component map: map [n][H][W] uint8 (map_bytes 1) or int32 (map_bytes 4: the components
 * of stswin_label_components, -1 = none), conf uint8 [n][H][W] -> out int64 [n][K][3].  Row out[f][i], over the pixels of frame f whose
 * map value is i, 0 <= i < K:    0: their number     1: the sum of conf     2: the number of them with conf < low
 * Other map values are counted nowhere.  out is written in full by the call (cleared by a fill kernel on the stream, no memset node):
 * a second call into the same out overwrites.  Two launches, no scratch buffer, no synchronisation, no allocation (graph-capturable).
 * Integer atomics only (exact, independent of the order: bit-reproducible).  A thread takes 16 consecutive pixels of a frame and adds a
 * run of equal values to its workgroup's LDS bins at once; non-zero bins go out with one 64-bit atomic each.  Any W: map and conf 16-byte
 * aligned with H W % 16 == 0 takes the body with 16-byte loads, anything else the element body.  1 <= H, W <= 16384, 1 <= K <= 1024,
 * 0 <= low <= 256.  The buffers must not overlap (the host wrapper checks).
 * Errors, before anything is launched: -1884 n, H or W <= 0, or H or W > 16384 (or more workgroups than a grid holds); -1885 map, conf
 * or out NULL; -1886 map_bytes not 1 or 4; -1887 K outside 1 .. 1024; -1888 low outside 0 .. 256; -1889 map not aligned to map_bytes or
 * out not 8-byte aligned. */
int stswin_confidence_sums(const void* map /*[n][H][W]*/, int map_bytes /*1: uint8, 4: int32*/, const unsigned char* conf /*[n][H][W]*/,
                           long long* out /*[n][K][3]*/, int K, int low, int n, int H, int W, void* stream);
/* ---- parts and contacts of the instances (stswincl_amd/utils/instruments.py instance_parts, VideoSegmenter(parts=...)): what an
 * instance is made of and what it touches.  labels uint8 [n][H][W], the model's labels (ungrouped, where VideoSegmenter(instance_groups=
 * ...) took the components of grouped ones); components int32 [n][H][W], the map of stswin_label_components, -1 = none.
 *   parts[f][i][c], 0 <= i < K, 0 <= c < nc: the ten integers of stswin_label_moments - count, sum x, sum y, sum x^2, sum xy, sum y^2,
 *       max(W - x), max(H - y), max(x + 1), max(y + 1) - over the pixels (y, x) of frame f with components == i and labels == c; all
 *       zero where there are none.
 *   contacts[f][i][c]: the number of ordered pairs (p, q), p a pixel of frame f with components[p] == i, q one of p's four neighbours
 *       inside the frame with components[q] != i and labels[q] == c: the length in pixel edges of the border between instance i and
 *       class c outside it, whatever the connectivity the components were taken with.  Borders between the parts of one instance are
 *       not counted; a neighbour of another instance, of a skipped class or of an ordinal >= K is counted under its label.
 * Pixels with ordinal -1 or >= K are nobody's p; labels >= nc count nowhere, neither in parts nor as q's class.  Both outputs are
 * written in full by the call (cleared by a fill kernel each on the stream, no memset node): a second call into the same outputs
 * overwrites.  Three launches, no scratch buffer, no allocation, no synchronisation (graph-capturable); integer atomics only (adds and
 * maxima: exact, independent of the order, bit-reproducible); no kernel waits on another workgroup.  A workgroup takes a tile of
 * stswin_instance_parts_geometry(0) x (1) pixels and reads each map once plus the one-pixel frame around the tile; a thread folds the
 * runs of equal (ordinal, class) along 16 pixels of a row and adds them to a keyed table of stswin_instance_parts_geometry(2) slots
 * on chip, whose slots in use go out with one 64-bit atomic per non-zero integer; a key that finds no slot among its probes - always
 * so once the table is full - adds to the outputs directly, with the same result.  Any W and any pointer: labels and components
 * 16-byte aligned with W % 16 == 0 takes the body with 16-byte loads, anything else the element body.  1 <= H, W <= 16384, 1 <= nc <=
 * 64, 1 <= K <= 1024; every sum fits an int64 and contacts <= 4 H W.  The buffers must not overlap (the host wrapper checks).
 * Errors, before anything is launched: -1890 n, H or W <= 0, or H or W > 16384 (or more workgroups than a grid holds); -1891 labels,
 * components, parts or contacts NULL; -1892 nc outside 1 .. 64; -1893 K outside 1 .. 1024; -1894 components not 4-byte aligned, or parts
 * or contacts not 8-byte aligned. */
int stswin_instance_parts(const unsigned char* labels /*[n][H][W]*/, const int* components /*[n][H][W]*/,
                          long long* parts /*[n][K][nc][10]*/, long long* contacts /*[n][K][nc]*/, int n, int H, int W, int nc, int K,
                          void* stream);
/* the geometry of stswin_instance_parts (the tests place their shapes around it): which = 0: the tile's height (32), 1: its width
 * (128), 2: the slots of the on-chip table (64); anything else: -1. */
int stswin_instance_parts_geometry(int which);
/* ---- clearance of the instances (stswincl_amd/utils/instruments.py instance_clearance, VideoSegmenter(clearance=...)): how near an
 * instance comes to what it does not touch.  labels uint8 [n][H][W] and components int32 [n][H][W] as for stswin_instance_parts ->
 * out int64 [n][K][nc][3].  For frame f, ordinal i < K and class c < nc, with I the pixels of components == i and Q those of labels == c:
 *   out[f][i][c] = (d2, p, q): d2 the smallest squared Euclidean pixel distance between a pixel of I and a pixel of Q; p = y W + x the
 *       smallest raster index among the pixels of I that reach d2; q the smallest raster index among the pixels of Q at d2 from p;
 *   out[f][i][c] = (-1, -1, -1) where I is empty, bit c of target_mask is clear, Q is empty, instance i itself holds a pixel of class
 *       c (an own class: with grouped components an arm's shaft, wrist and clasper; a plane per class cannot leave an instance's own
 *       pixels out, so the distance between two instances of one class is not measured), or max_d2 >= 0 and d2 > max_d2.
 * Ordinals -1 and >= K are nobody's, labels >= nc are nowhere.  max_d2 = -1: no limit.  out is written in full by the call (by the last
 * launch; nothing needs clearing beforehand, a second call overwrites).  workspace: caller-owned, 8-byte aligned, >=
 * stswin_instance_clearance_scratch(n, H, W, nc, K) = 8 n (S W + 1 + K nc + K) + n H W (2 nc + 1) bytes with S = ceil(H / 64) (the
 * segment table uint64 [n][S][W] and the maps' classes uint64 [n] of stswin_boundary_counts; the keys uint64 [n][K][nc]; the classes
 * each instance holds, uint64 [n][K]; the column distances uint16 [n][nc][H][W]; the contour codes uint8 [n][H][W]); nothing in it needs
 * clearing (fill kernel on the stream, no memset node) and nothing survives the call.  Six launches whatever nc, K and the maps hold -
 * fill; mark the contours of the target classes and the classes each instance holds; classes per segment and column distances, the
 * two kernels of stswin_boundary_counts over n maps; query: every pixel of an instance with a 4-neighbour of another ordinal or
 * outside the image (a nearest pixel always is one) searches the plane of every present target class its instance does not hold,
 * bounded by the pair found so far (alone up to 8 columns, then the wave for one pixel at a time or for the whole row at once), and lowers the 64-bit key d2 2^28 + p by an atomic minimum; resolve: a wave per (f, i, c) finds q
 * on the circle of radius^2 d2 around p - no synchronisation, no allocation, no host read (graph-capturable); no kernel waits on
 * another workgroup.  Integer arithmetic and integer atomics only (or, min): exact, independent of the order (bit-reproducible); float
 * square roots only seed integer roots, integer comparisons decide them.  components 4-byte and out 8-byte aligned, labels at any
 * address, any W; 1 <= H, W <= 16384 (d2 < 2^30, p < 2^28), 1 <= nc <= 64, 1 <= K <= 1024.  The buffers must not overlap (the host
 * wrapper checks).
 * Errors, before anything is launched: -1920 n, H or W <= 0, or H or W > 16384 (or more workgroups than a grid holds; also what
 * stswin_instance_clearance_scratch returns for such a shape); -1921 labels, components, out or workspace NULL; -1922 nc outside 1 ..
 * 64 and -1923 K outside 1 .. 1024 (both from stswin_instance_clearance_scratch too); -1924 workspace_bytes too small or workspace not
 * 8-byte aligned; -1925 components not 4-byte or out not 8-byte aligned; -1926 max_d2 < -1. */
long stswin_instance_clearance_scratch(int n, int H, int W, int nc, int K);
int stswin_instance_clearance(const unsigned char* labels /*[n][H][W]*/, const int* components /*[n][H][W]*/,
                              long long* out /*[n][K][nc][3]*/, int n, int H, int W, int nc, int K, long target_mask, long max_d2,
                              void* workspace, long workspace_bytes, void* stream);
/* the geometry of stswin_instance_clearance (the tests place their shapes around it): which = 0 .. 3: what stswin_boundary_geometry
 * gives (the query tile 16 x 64, the columns of a workgroup and the rows of a segment of the column pass, 64 and 64); 4: the columns
 * a lane searches to each side on its own before the wave searches together, 64 columns a step (8); 5: the pixels of a row the near
 * search may leave over for the wave to take one by one (2) - more of them search at once, each column loaded once for all;
 * anything else: -1. */
int stswin_instance_clearance_geometry(int which);
/* ---- the label map cleaned: specks out, small holes filled (stswincl_amd/utils/instruments.py clean_labels states the result bit
 * for bit; VideoSegmenter(clean_area=A)).  labels uint8 [n][H][W] -> out uint8 [n][H][W], stats int32 [n][2].
 *   The components of every class c < nc, nothing skipped, under `connectivity` 4 or 8, are those of stswin_label_components; pixels
 *   with a label >= nc belong to none, are never changed and never vote.  A component is small if its area is < min_area and its class
 *   is not in `keep` (bit c of the mask: class c is kept); every other pixel of a class < nc is stable.  A frame's small components are
 *   numbered s = 0, 1, ... by their first pixel in raster order; only those with s < max_small can be relabelled, the rest stay as they
 *   are whatever the order of execution, but still count as small.  votes[s][c] = the number of ordered pairs (p, q), p a pixel of
 *   small component s, q one of p's four neighbours inside the frame, stable, with labels[q] == c (always the input labels: one pass).
 *   The new label of s is the smallest c with the largest votes[s][c] if that is > 0, else its own.
 *   stats[f] = (the frame's number of small components, not bounded by max_small; the number of pixels whose label changed).
 * out and stats are written in full; nothing in the workspace needs clearing by the caller (what is accumulated is cleared by fill
 * kernels on the stream, no memset node).  No allocation, no synchronisation (graph-capturable); no kernel waits on another workgroup;
 * integer atomics only (exact, independent of the order: bit-reproducible).  workspace: caller-owned, 4-byte aligned, >=
 * stswin_labels_clean_scratch(n, H, W, nc, max_small) bytes (two int32 maps, the chunk counts, and per frame max_small (2 + nc) words).
 * Twelve launches: two fills (the areas, the votes); the tile, border (more than one tile only) and root pass of
 * stswin_label_components with an empty skip mask, after which the parent map holds every pixel's root; areas by root, a thread
 * folding the runs along 16 pixels of a row and a workgroup gathering its tile's runs on chip before the atomics; the count of small roots per raster chunk, its scan and the numbering
 * (which also writes stats); the vote pass, in which only pixels of small components with s < max_small do any work, a workgroup
 * gathering the votes of its tile of stswin_labels_clean_geometry(0) x (1) pixels in a keyed on-chip table of (3) slots and adding
 * directly where a key finds no slot; the resolve pass, a thread per small component; the relabel pass.  Any pointer alignment, any W:
 * labels, out and workspace 16-byte aligned with W % 16 == 0 takes the bodies with 16-byte loads and stores, anything else the element
 * bodies.  1 <= H, W <= 16384.  out must not overlap labels (the host wrapper checks).
 * Errors, before anything is launched: -1900 n, H or W <= 0, or H or W > 16384, or more workgroups than a grid holds
 * (stswin_labels_clean_scratch returns the same for such a shape); -1901 labels, out, stats or workspace NULL; -1902 nc outside 1 ..
 * 64; -1903 connectivity not 4 or 8; -1904 min_area outside 2 .. 2^30; -1905 max_small outside 1 .. 65536; -1906 workspace too small
 * or not 4-byte aligned (or stats not 4-byte aligned). */
long stswin_labels_clean_scratch(int n, int H, int W, int nc, int max_small);
int stswin_labels_clean(const unsigned char* labels /*[n][H][W]*/, unsigned char* out /*[n][H][W]*/, int* stats /*[n][2]*/, int n, int H,
                        int W, int nc, int connectivity, long keep, int min_area, int max_small, void* workspace, long workspace_bytes,
                        void* stream);
/* the geometry of stswin_labels_clean (the tests place their shapes around it): which = 0: the vote tile's height (32), 1: its width
 * (128), 2: the pixels of a raster chunk of the numbering pass (2048), 3: the slots of the on-chip vote table (256); anything else: -1. */
int stswin_labels_clean_geometry(int which);
/* what the fused label launches count, from a label map that already exists (a cleaned one): labels uint8 [n][H][W], gt int64
 * [n][H][W].  With counts (int32 [n][3][nc], zeroed by the caller): counts[f][0 | 1 | 2][c] += |gt == c|, |labels == c|, |gt == c and
 * labels == c|, the integers of stswin_upsample_argmax.  With cm (int64 [ncm][ncm]): every pixel with 0 <= gt < ncm and labels < ncm
 * adds 1 to cm[gt][labels]; accumulated, never cleared, as stswin_upsample_argmax_cm does.  Either or both.  One launch: LDS bins per
 * workgroup, one atomic per non-zero bin; integer adds only.  gt 8-byte aligned, labels at any address.
 * Errors: -1910 n, H or W <= 0, or H or W > 16384; -1911 labels or gt NULL, or counts and cm both NULL; -1912 nc outside 1 .. 64, or
 * (with cm) ncm outside 1 .. 64; -1913 gt or cm not 8-byte aligned, or counts not 4-byte aligned. */
int stswin_labels_score(const unsigned char* labels /*[n][H][W]*/, const long long* gt /*[n][H][W]*/, int* counts /*[n][3][nc] or NULL*/,
                        unsigned long long* cm /*[ncm][ncm] or NULL*/, int ncm, int n, int H, int W, int nc, void* stream);
/* ---- frames as a video source delivers them (stswincl_amd/utils/yuv.py, VideoSegmenter(pixel_format=..., out_format="nv12")):
 * stswin_yuv_to_rgb makes the HWC RGB frame uint8 [n][Hs][Ws][3] that stswin_frame_ingest and stswin_labels_overlay read,
 * stswin_rgb_to_nv12 turns such a frame into NV12.  Hs (NV12) and Ws are even.
 *   format 0, nv12: uint8 [n][3 Hs / 2][Ws]; rows 0 .. Hs-1 are luma, rows Hs .. are Hs / 2 rows of Ws / 2 interleaved (U, V) pairs.
 *   format 1, uyvy: uint8 [n][Hs][Ws][2]; the four bytes of pixel pair (2k, 2k+1) are U, Y0, V, Y1.
 * matrix is int32 [3][4] in device memory (utils.yuv.to_rgb_matrix / to_yuv_matrix): per output channel three coefficients in
 * units of 2^-14 and an offset that holds the rounding half.  A triple t gives
 *     out_c = clamp((m[c][0] t0 + m[c][1] t1 + m[c][2] t2 + m[c][3]) >> 14, 0, 255)      (arithmetic shift: a floor; int32 suffices)
 * with t = (Y, U, V) -> (R, G, B) for stswin_yuv_to_rgb and t = (R, G, B) -> (Y, U, V) for stswin_rgb_to_nv12.
 * Chroma of a pixel, C[j][k] one chroma plane:
 *   chroma 0, replicate: pixel (y, x) uses C[y >> 1][x >> 1] (nv12) or C[y][x >> 1] (uyvy).
 *   chroma 1, linear (MPEG-2 siting: co-sited with the even columns, vertically centred): nv12 first interpolates vertically,
 *     row 2j: V[k] = (3 C[j][k] + C[max(j-1, 0)][k] + 2) >> 2, row 2j+1: V[k] = (3 C[j][k] + C[min(j+1, Hs/2 - 1)][k] + 2) >> 2
 *     (uyvy: V is the row's own chroma); then both formats horizontally, x = 2k: V[k], x = 2k+1: (V[k] + V[min(k+1, Ws/2 - 1)] + 1) >> 1.
 * stswin_rgb_to_nv12: luma per pixel from its own RGB through row 0; chroma through rows 1 and 2 from the 2 x 2 block's per-channel
 * mean (sum of four + 2) >> 2.
 * Each is one launch, no scratch buffer, no synchronisation, no atomics (graph-capturable).  Any pointer alignment, any even size:
 * Ws % 8 == 0 with the pointers 8-byte (uyvy in: 16-byte) aligned takes the body with 8 pixels per thread and row (nv12: of both luma
 * rows of a chroma row), anything else the body with 2.  Integer arithmetic only.
 * Errors (both): -1424 n, Hs or Ws <= 0; -1425 in, matrix or out NULL; -1426 odd Ws, or odd Hs (nv12, stswin_rgb_to_nv12);
 * -1427 format outside 0 .. 1; -1428 chroma outside 0 .. 1; -1429 out overlaps in (or matrix). */
int stswin_yuv_to_rgb(const unsigned char* in, const int* matrix, unsigned char* out, int n, int Hs, int Ws, int format, int chroma,
                      void* stream);
int stswin_rgb_to_nv12(const unsigned char* in, const int* matrix, unsigned char* out, int n, int Hs, int Ws, void* stream);

/* ---- video inference (stswincl_amd/video.py), the evaluation loop of seg18/test.py:147-175 over the clips of
 * seg18/dataset/Endovis2018_new.py:109-127.
 * stswin_frame_ingest: uint8 RGB frames in [n][Hs][Ws][3] (HWC) -> fp32 images out [n][3][H][W], the stem's input
 * (Endovis2018_new.py:125-127 `Image.resize((W, H), Image.BILINEAR)`, then `astype(float) / 255.` and test.py:149 `.float()`).
 * Bit-exact with Pillow's separable BILINEAR resampler: when Ws != W a horizontal pass writes the uint8 intermediate
 * tmp [n][Hs][W][3] (caller-owned), then when Hs != H a vertical pass; per output index i the taps are [bounds[2i],
 * bounds[2i] + bounds[2i+1]) with int32 weights coef[i][ksize] of 22 fraction bits, out = clip((2^21 + sum u * k) >> 22, 0, 255).
 * The tables are the caller's (float64 on the host); a pass whose size is unchanged needs none.  lut[256] maps the byte
 * to its fp32 value (float32(u / 255.)).  Integer arithmetic only.
 * stswin_clip_assemble: clips [B][4][frame_elems] from a frame-feature ring [slots][frame_elems] and this step's fresh frame
 * features [n_fresh][frame_elems] (the T = 4 frames of base18.py:86-89 computed once per frame): table (int32, device) holds B*4
 * sources, >= 0 = ring slot, < 0 = fresh frame -1 - e, then n_store ring slots that fresh frames 0 .. n_store-1 are stored
 * into (< 0 = not kept).  A source out of range yields zeros, a store out of range is skipped.  No slot may be both read and
 * stored by one call.  frame_elems * sizeof(dtype) % 16 == 0. */
int stswin_frame_ingest(const unsigned char* in, unsigned char* tmp, float* out, int n, int Hs, int Ws, int H, int W,
                        const int* hbounds, const int* hcoef, int hksize, const int* vbounds, const int* vcoef, int vksize,
                        const float* lut, void* stream);
/* stswin_frame_ingest_planes: stswin_frame_ingest with one value table per RGB plane, lut [3][256] (the CaDIS transform,
 * segcata/dataset/CATA_new_512.py:21-22, 228-229: float32((u / 255. - MEAN[c]) / STD[c]) computed in float64 on the host). */
int stswin_frame_ingest_planes(const unsigned char* in, unsigned char* tmp, float* out, int n, int Hs, int Ws, int H, int W,
                               const int* hbounds, const int* hcoef, int hksize, const int* vbounds, const int* vcoef, int vksize,
                               const float* lut, void* stream);
int stswin_clip_assemble(int dtype, void* ring, const void* fresh, void* clips, const int* table, int B, int n_store, int slots,
                         int n_fresh, long frame_elems, void* stream);

/* ---- training input (stswincl_amd/augment.py): the transform of seg18/dataset/Endovis2018_new.py:61-107, 145-182 (random scale,
 * pad, crop, flips, brightness / contrast, rotate, / 255.) on uint8 clips [B][T][Hs][Ws][3] and uint8 labels [B][Hs][Ws], in two
 * stages.  Integer arithmetic until the last table lookup: every output is defined bit for bit.  What is random is drawn on the
 * host and arrives as one row per sample of each stage's int32 table (device memory, row stride table_stride words).  No allocation, no
 * synchronisation, no memset: every output element is written by a kernel on the caller's stream.
 *
 * stswin_augment_crop: scale + pad + crop + flip.  Pillow's separable BILINEAR (as stswin_frame_ingest: taps [first, first + n),
 * int32 weights of 22 fraction bits, uint8 intermediate, out = clip((2^21 + sum u * k) >> 22, 0, 255)) evaluated for the Wc columns
 * and Hc rows of the crop window only.  tmp is the caller's uint8 intermediate [B][T][Hs][Wc][3]; crop [B][T][Hc][Wc][3] and
 * label_crop [B][Hc][Wc] are the outputs.  A sample's table row, in words (stswin_augment_crop_table_stride gives the length):
 *     r0, r1, flags, 0        the horizontal pass covers source rows [r0, r1); flags: 1 = horizontal flip, 2 = vertical flip
 *     hbounds [Wc][2]         (first tap, taps) per window column; taps = 0: padding (the pixel is 0); an unscaled axis has one
 *     hcoef   [Wc][ksize]      tap of weight 2^22 per index
 *     vbounds [Hc][2], vcoef [Hc][ksize]     the same per window row
 *     lx [Wc], ly [Hc]        the label's source column / row (Pillow NEAREST), < 0: padding (label 0)
 * The flips are applied at the store: window pixel (y, x) is written to (flags & 2 ? Hc-1-y : y, flags & 1 ? Wc-1-x : x).
 *
 * stswin_augment_finish: value table + rotate + convert.  crop / label_crop as above -> images fp32 [B][T][3][Hc][Wc] and labels
 * int64 [B][Hc][Wc].  A sample's table row (stswin_augment_finish_table_stride words):
 *     flags, key0, key1, noise     flags: 1 = rotate; words 1 .. 3 belong to stswin_augment_noise (this stage never reads them)
 *     colx [Wc], coly [Wc], rowx [Hc], rowy [Hc]     int32 positions with 10 fraction bits
 *     bc [64]                 the sample's uint8 -> uint8 value table (256 bytes; identity when unused), applied to every source
 *                             pixel before the interpolation
 * Rotation: the source position of output (y, x) is X = (rowx[y] + colx[x]) >> 5, Y = (rowy[y] + coly[x]) >> 5 in 1/32 pixel;
 * with fx = X & 31, fy = Y & 31 the weights are (32-fx | fx) x (32-fy | fy) over the pixels (X >> 5 | +1, Y >> 5 | +1), indices
 * reflected (reflect-101), out = (sum w v + 512) >> 10; the label reads the pixel ((X + 16) >> 5, (Y + 16) >> 5), reflected.
 * Without the flag the sample copies through.  Then plane c of the image is lut[c * (lut_planes ? 256 : 0) + v] (fp32 [256] or
 * [3][256]) and the label is label_lut[l] (int64 [256]).
 *
 * stswin_augment_noise: CaDIS's Gaussian noise (segcata/dataset/CATA_new_512.py:178-183: skimage random_noise(mode='gaussian',
 * var=0.001, clip=True), stored as (255 * clip(u / 255. + n, 0, 1)).astype('uint8')), between the two stages, in place on stage 1's
 * crop taken as [B][sample_bytes] (sample_bytes = T Hc Wc 3, a multiple of 4).  For a byte u that expression is
 * clamp(u + floor(255 n), 0, 255): an integer offset K with the law P(K <= k) = Phi((k + 1) / (255 sqrt(var))), which the host
 * states as n_thr ascending uint32 thresholds thr (device memory) and k_min.  `table` is the stage-2 table above: a sample with
 * noise != 0 is switched on and (key0, key1) is its 64-bit key, low word first; a sample with noise == 0 is not written at all.
 * Per byte i of a noisy sample:
 *     w[0..3] = Philox4x32-10(counter = (i >> 2, 0, 0, 0), key = (key0, key1))        r = w[i & 3]
 *     K       = k_min + #{ j < n_thr : thr[j] <= r }
 *     out     = clamp(u + K, 0, 255)
 * Philox4x32-10 as published (Salmon et al., Random123): multipliers 0xD2511F53 and 0xCD9E8D57, key increments 0x9E3779B9 and
 * 0xBB67AE85 per round, ten rounds.  The noise of a byte is a function of (key, i) alone - the reference's own stream is unseeded
 * and cannot be reproduced.  Any pointer alignment: 16-byte accesses where the address allows them, bytes elsewhere.  Integer
 * arithmetic only; one launch, no allocation, no synchronisation, no memset.
 * Errors, before anything is launched: -1808 B <= 0, sample_bytes <= 0, not a multiple of 4 or > 2^34; -1809 crop, table or thr
 * NULL; -1810 n_thr outside 1 .. 1024; -1819 table_stride < stswin_augment_finish_table_stride(1, 1), the shortest stage-2 row. */
long stswin_augment_crop_table_stride(int Hc, int Wc, int ksize);
int stswin_augment_crop(const unsigned char* frames, const unsigned char* labels, unsigned char* tmp, unsigned char* crop,
                        unsigned char* label_crop, const int* table, long table_stride, int ksize, int B, int T, int Hs, int Ws,
                        int Hc, int Wc, void* stream);
long stswin_augment_finish_table_stride(int Hc, int Wc);
int stswin_augment_finish(const unsigned char* crop, const unsigned char* label_crop, float* images, long* labels_out,
                          const int* table, long table_stride, const float* lut, int lut_planes, const long* label_lut, int B,
                          int T, int Hc, int Wc, void* stream);
int stswin_augment_noise(unsigned char* crop, const int* table, long table_stride, const unsigned int* thr, int n_thr, int k_min,
                         int B, long sample_bytes, void* stream);

/* ---- contrastive pre-training input (stswincl_amd/contrast/views.py): the six RandomResizedCropCoord + RandomHorizontalFlipCoord +
 * ToTensor + Normalize pipelines of pixcontrast_18/contrast/data/dataset.py:43-70 (contrast/data/transform.py:20-87,
 * transform_coord.py:81-224) on the uint8 frames [F][Hs][Ws][3] and uint8 labels [L][Hs][Ws] of a batch as they are stored.
 * stswin_contrast_views writes V = views x samples output view-samples: images fp32 [V][4][3][H][W] and masks fp32 [V][1][H][W]
 * (the form stswin_labels_resize reads).  Pillow's crop + separable BILINEAR resize as stswin_augment_crop computes it (taps
 * [first, first + n), int32 weights of 22 fraction bits, out = clip((2^21 + sum u * k) >> 22, 0, 255), an unscaled axis has one tap of
 * weight 2^22): the horizontal pass writes rows [r0, r1) of the four frames into the caller's uint8 tmp [V][4][Hs][W][3], the vertical
 * pass stores plane c as lut[c][v] (lut fp32 [3][256]) at the flipped address, and mask (y, x) = float(label[ly[y]][lx[x]]) (Pillow
 * NEAREST).  A view-sample's row of the int32 device table (row stride table_stride words, stswin_contrast_views_table_stride gives
 * the length):
 *     r0, r1, flags, label    source rows [r0, r1) of the horizontal pass; flags: 1 = horizontal flip, 2 = vertical flip; label: index
 *                             into labels [L]
 *     frame [4]               indices into frames [F] of the clip's four frames, in output order (views may share frames)
 *     hbounds [W][2], hcoef [W][ksize], vbounds [H][2], vcoef [H][ksize]     (first tap, taps) and weights per output column / row,
 *                             in source coordinates
 *     lx [W], ly [H]          the label's source column / row
 * ksize <= 16.  Window pixel (y, x) is written to (flags & 2 ? H-1-y : y, flags & 1 ? W-1-x : x).  Frame, label, tap and label
 * coordinates outside their source are clamped into it (the host wrapper refuses them).  No allocation, no synchronisation, no
 * memset: two launches on the caller's stream write every output element. */
long stswin_contrast_views_table_stride(int H, int W, int ksize);
int stswin_contrast_views(const unsigned char* frames, const unsigned char* labels, unsigned char* tmp, float* images, float* masks,
                          const int* table, long table_stride, const float* lut, int ksize, int V, int F, int L, int Hs, int Ws,
                          int H, int W, void* stream);

/* ---- f2: multi-tensor optimizer / EMA step, up to 48 fp32 tensors per launch (host arrays of device pointers).
 * mode 0 = torch.optim.Adam (seg18/train_swin.py:122; c1 = 1 - b1^t, c2 = sqrt(1 - b2^t)), 1 = torch.optim.SGD with
 * momentum b1 (train_CL_ft_mswin_sgd_minput.py:147-162; c1 != 0 marks the first step: buf = grad), 2 = EMA
 * p = p*b1 + g*(1-b1) with g = the query parameter (PixPro_swin_v5.py:258-289). */
int stswin_multi_tensor(int mode, int count, void* const* p, const void* const* g, void* const* m, void* const* v,
                        const int* n, float lr, float b1, float b2, float eps, float wd, float c1, float c2, void* stream);

/* LARS over SGD-momentum (pixcontrast_18/contrast/lars.py:109-152 wrapping torch.optim.SGD, main_pretrain_swinv5.py:37-47) for up
 * to 48 fp32 tensors of ONE parameter group, three launches: per-block partial ||p||^2 and ||g + wd p||^2, their fixed-order fold
 * into `norms` (caller-owned fp32 scratch, norms_floats >= 2 * count + 2 * sum_i ceil(n_i / 8192); no atomics: reproducible), then g' = (g + wd p) * (adaptive && both norms > 0 ? trust_coef ||p|| / (||g'|| + eps) : 1),
 * buf = first ? g' : momentum * buf + g', p -= lr * buf.  adaptive = 0: the 'ignore' group of add_weight_decay (biases, norms). */
int stswin_multi_tensor_lars(int count, void* const* p, const void* const* g, void* const* m, const int* n, float* norms,
                             long norms_floats, float lr, float momentum, float wd, float trust_coef, float eps, int first, int adaptive,
                             void* stream);

/* Step-dependent optimizer scalars in DEVICE memory, so that a hipGraph replay of a training step advances like eager steps do
 * (the reference's loops step Adam / LARS / the key-encoder momentum from host state every iteration: seg18/train_swin.py:122,171-173,
 * pixcontrast_18/main_pretrain_swinv5.py:37-47, contrast/models/PixPro_swin_v5.py:258-289).  hyper = fp32 [4] {lr, c1, c2, EMA momentum}.
 * stswin_optim_tick (one thread, double precision like the host expressions it replaces):
 *   kind 0: t = ++counter[0]; hyper[1] = 1 - a^t; hyper[2] = sqrt(1 - b^t)                   (Adam bias corrections, a, b = betas)
 *   kind 1: k = counter[0]++; hyper[3] = 1 - (1 - a) (cos(pi k / b) + 1) / 2                  (PixPro_swin_v5.py:260; a = base momentum, b = K)
 * stswin_multi_tensor_dev / stswin_multi_tensor_lars_dev: stswin_multi_tensor / stswin_multi_tensor_lars reading lr (hyper[0]), the Adam
 * corrections (hyper[1], hyper[2]) or the EMA momentum (hyper[3]) from `hyper` instead of their arguments; `first` as c1 != 0 above.
 * hyper[0] is written by the host with a stream-ordered fill whenever the scheduler changes the learning rate. */
int stswin_optim_tick(int kind, int* counter, float* hyper, double a, double b, void* stream);
int stswin_multi_tensor_dev(int mode, int count, void* const* p, const void* const* g, void* const* m, void* const* v, const int* n,
                            const float* hyper, float b1, float b2, float eps, float wd, int first, void* stream);
int stswin_multi_tensor_lars_dev(int count, void* const* p, const void* const* g, void* const* m, const int* n, float* norms,
                                 long norms_floats, const float* hyper, float momentum, float wd, float trust_coef, float eps, int first,
                                 int adaptive, void* stream);

/* ---- device self-test of the MFMA / LDS primitives the kernels are built on; writes a report into `out`
 * (fp32, >= 64 KiB) and returns the number of failed checks (0 = all good). Used by tests only. */
int stswin_selftest(float* out, int which, void* stream);
/* In-run calibration probes of bench.py (measurement infrastructure, never on the product path): stswin_calib_mfma launches 256
 * workgroups of `waves_per_cu` waves, each running `iters` rounds of 8 independent v_mfma_f32_16x16x32_bf16, and returns the MFMA
 * instructions per round of the whole launch (flops = that x iters x 16384); stswin_calib_copy copies `bytes` with 16-byte lanes. */
long stswin_calib_mfma(int waves_per_cu, int iters, float* sink, void* stream);
int stswin_calib_copy(const void* src, void* dst, long bytes, void* stream);
/* Measurement stand-in for an RCCL all-reduce of one gradient bucket as the main stream sees it (tools/overlap_proxy.py): `workgroups`
 * workgroups of 256 threads copy src -> dst (`bytes`, 16-byte pieces) `passes` times, i.e. hold that many compute units for that long.
 * No peer traffic; never on the product path. */
int stswin_proxy_collective(const void* src, void* dst, long bytes, int workgroups, int passes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
