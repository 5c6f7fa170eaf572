/* runet_hip.h — C ABI of librunet_hip.so: the gfx950 (MI355X) kernels behind the Robust U-Net
 * training path.
 *
 * Every entry point is `extern "C"`, takes plain device pointers + sizes + a HIP stream handle
 * (`void* stream` = hipStream_t; NULL = default stream), launches asynchronously on that stream,
 * allocates nothing, keeps no global state (except the thread-local last-error string) and returns
 * 0 on success / non-zero on error (`runet_last_error()` has the text).  Arguments are validated
 * on the host before any launch: a bad shape is an error code, never an out-of-bounds kernel.
 *
 * The reference (UofgCoastline/EUSIPCO-2026-Robust-Unet) is pure Python on top of torch; it has no
 * FFI of its own.  Each group below names the reference call site(s) (file:line in /root/reference)
 * whose ATen kernels it stands in for; the Python binding that a maintainer of the reference would
 * add is shown in INTEGRATION.md (ctypes) and implemented in eusipco-2026-robust-unet_amd/_lib.py.
 *
 * Layouts: activations are NHWC fp32; `ld*` is the pixel stride in floats, so a tensor may be a
 * channel slice of a wider (concat) buffer.  Convolution weights are "HWIO": w[kh][kw][cin][cout].
 */
#ifndef RUNET_HIP_H
#define RUNET_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

const char* runet_last_error(void);
void runet_set_error(const char* msg);
int runet_abi_version(void);

/* ---- convolutions (Main_Final.py:157,159,172 ResidualBlock; :126,131 AttentionGate 1x1; :205-208
 *      DilatedBlock; :261-270 ConvTranspose2d k2 s2; autograd of the same via :581 loss.backward()) ---- */
enum { RUNET_CONV_FWD = 0, RUNET_CONV_DGRAD = 1, RUNET_CONVT_FWD = 2, RUNET_CONVT_DGRAD = 3, RUNET_CONV_DGRAD_T = 4, RUNET_CONVT_DGRAD_T = 5 };

/* mode FWD   : y[n,h,w,0:cout] (=|+=) bias + conv_{kh x kw, dilation dil, 'same' zero padding}(x[n,h,w,0:cin], w[kh,kw,cin_w,cout])
 *              cin is the channel count READ from x (multiple of 4, zero-padded by the caller);
 *              cin_w <= cin is the number of input channels present in w (3 for the RGB stem).
 * mode DGRAD : x := dy[n,h,w,0:cin] (cin = conv Cout), y := dx[n,h,w,0:cout] (cout = conv Cin),
 *              w = the forward weight [kh,kw,cout,cin]; computes the data gradient.
 * mode CONVT_FWD  : y[n,2h,2w,0:cout] = bias + convT_{2x2,s2}(x[n,h,w,0:cin]),  w[2,2,cin,cout]
 * mode CONVT_DGRAD: x := dy[n,2h,2w,0:cin], y := dx[n,h,w,0:cout],  w[2,2,cout,cin]
 * modes DGRAD_T / CONVT_DGRAD_T: the same data gradients with the weight already transposed per tap, w [taps][cin][cout] in THIS call's
 *              naming (runet_transpose_taps of the forward weight, cached per optimizer step): the weight tile is then staged with the
 *              n-contiguous loader of the forward kernels instead of the k-contiguous one (scalar LDS writes).
 * accumulate != 0 adds into y instead of overwriting.  bias may be NULL. */
int runet_conv_igemm(const float* x, int ldx, const float* w, const float* bias, float* y, int ldy,
                     int n_img, int h, int w_, int cin, int cin_w, int cout, int kh, int kw, int dil,
                     int mode, int accumulate, void* stream);

/* wt[tap][co][ci] = w[tap][ci][co] */
int runet_transpose_taps(const float* w, float* wt, int taps, int cin, int cout, void* stream);

/* name of the kernel instantiation runet_conv_igemm launches for this shape (as rocprofv3 prints it, minus the
 * namespace), so that bench.py's live timings can be matched with the profiler's per-kernel rows */
const char* runet_conv_igemm_kernel_name(int n_img, int h, int w_, int cin, int cout, int kh, int mode);
/* measurement hook (tools/igemm_variants.py): force the tile variant of runet_conv_igemm, 0..4 = 128x32, 256x64, 128x64, 128x128, 64x64; -1 = automatic */
int runet_igemm_force_variant(int variant);
/* the same for runet_conv_igemm_bf16 / _fp16: 0..2 = 128 pixels x 32, 64, 128 output channels; -1 = automatic */
int runet_igemm_lowp_force_variant(int variant);

/* dw[kh,kw,cin_w,cout] = sum_pixels x (x) dy  (weight gradient; transposed != 0: dy is [n,2h,2w,cout]
 * and the 2x2 taps index the dy pixel).  `workspace` (>= runet_conv_wgrad_workspace_floats floats, may be
 * NULL) holds split-K partial slabs that are summed in a fixed order. */
long runet_conv_wgrad_workspace_floats(int n_img, int h, int w_, int cin_w, int cout, int kh, int kw);
int runet_conv_wgrad(const float* x, int ldx, const float* dy, int ldy, float* dw, float* workspace,
                     long workspace_floats, int n_img, int h, int w_, int cin, int cin_w, int cout,
                     int kh, int kw, int dil, int transposed, void* stream);


/* ---- Winograd F(2x2,3x3) path for the 3x3 / dilation-1 / 'same' convolutions (Main_Final.py:157,159), forward and data gradient ----
 * runet_wino_weights: U[16][K][N] = G g G^T of w[3][3][cin][cout]; dgrad = 0: K = cin, N = cout;  dgrad != 0: the 180-degree rotated
 * filter with K = cout, N = cin (so that runet_wino_conv(dy, U') is the data gradient).
 * runet_wino_conv: y[n,h,w,0:N] (=|+=) bias + winograd_conv(x[n,h,w,0:K], U).  Needs H, W even, K % 16 == 0, N even. */
int runet_wino_supported(int h, int w, int cin, int cout);
/* shape supported AND the tensors fit the kernel's 32-bit buffer offsets (n_img*h*w*ld < 2^29 floats): callers fall back to
 * runet_conv_igemm (64-bit addressing) when this is 0, e.g. 16 x 512 x 512 with a 128-channel concat input */
int runet_wino_fits(int n_img, int h, int w, int ldx, int ldy, int cin, int cout);
int runet_wino_weights(const float* w_hwio, float* U, int cin, int cout, int dgrad, void* stream);
int runet_wino_conv(const float* x, int ldx, const float* U, const float* bias, float* y, int ldy, int n_img, int h, int w, int k, int n,
                    int accumulate, void* stream);

/* The same convolution with its sixteen position products on the BF16 matrix cores (csrc/conv_winograd_x3.hip: split operands, six bf16
 * MFMAs per fp32 product, fp32-accurate).  runet_wino_weights_x3 writes G g G^T straight into the split planes Up[16][3][K/8][N][8] bf16
 * (runet_wino_x3_pack_elems(K, N) 2-byte elements, once per optimizer step); runet_wino_conv_x3 = runet_wino_conv on them (ldx % 4 == 0,
 * x 16-byte aligned). */
long runet_wino_x3_pack_elems(int k, int n);
int runet_wino_weights_x3(const float* w_hwio, void* Upacked, int cin, int cout, int dgrad, void* stream);
int runet_wino_conv_x3(const float* x, int ldx, const void* Upacked, const float* bias, float* y, int ldy, int n_img, int h, int w, int k, int n,
                       int accumulate, void* stream);
/* ... and with the BatchNorm statistics of its output (Main_Final.py:158,160: the BatchNorm2d behind each convolution) taken in the epilogue
 * instead of by a pass of runet_bn_stats over the tensor: stats [runet_wino_conv_x3_stats_parts(n_img, h, w)][n][3] = (count, mean, M2) per
 * block of pixels; runet_bn_stats_finalize turns them into the coefficients (the second kernel of runet_bn_stats). */
int runet_wino_conv_x3_stats_parts(int n_img, int h, int w);
int runet_wino_conv_x3_stats(const float* x, int ldx, const void* Upacked, const float* bias, float* y, int ldy, int n_img, int h, int w, int k,
                             int n, int accumulate, float* stats, void* stream);

/* Winograd-domain weight gradient of the same convolutions: dw[3][3][cin][cout] = G^T [sum_tiles (B^T x B).*(A dy A^T)] G.
 * workspace: >= runet_wino_wgrad_workspace_floats floats (partial slabs, summed in a fixed order).  H, W even. */
long runet_wino_wgrad_workspace_floats(int n_img, int h, int w, int cin, int cout);
int runet_wino_wgrad(const float* x, int ldx, const float* dy, int ldy, float* dw, float* workspace, long workspace_floats, int n_img,
                     int h, int w, int cin, int cout, void* stream);

/* ---- channel statistics / BatchNorm2d / ReLU / Dropout2d (Main_Final.py:158,160,162,163,173,127,132,137,210,211) ----
 * Scratch buffers ("workspace") are caller-owned; runet_reduce_workspace_floats gives a sufficient size. */
long runet_reduce_workspace_floats(int n_img, int hw, int c);

/* per-(image, channel) mean and M2 (= sum of squared deviations) of x[n, hw, 0:c]; optionally max/min and the
 * pixel index (within the image) of their first occurrence.  c is 1 or a multiple of 4, <= 1024. */
int runet_chan_stats(const float* x, int ld, int n_img, int hw, int c, float* workspace, float* mean_nc, float* m2_nc,
                     float* max_nc, float* min_nc, int* imax_nc, int* imin_nc, int want_minmax, void* stream);

/* training != 0: batch statistics over n_img*hw values from (mean_nc, m2_nc); updates run_mean/run_var (momentum,
 * unbiased variance) and *num_batches_tracked += 1 when those pointers are non-NULL; writes save_mean/save_invstd.
 * training == 0: statistics = run_mean/run_var.  Outputs scale = gamma*invstd, shift = beta - mean*scale. */
/* coefficients from statistics partials part[nparts][c][3] = (count, mean, M2) of disjoint pixel sets (written by runet_conv_x3_stats /
 * runet_wino_conv_x3_stats): the second kernel of runet_bn_stats on its own */
int runet_bn_stats_finalize(const float* part, int nparts, int c, const float* gamma, const float* beta, float* run_mean, float* run_var,
                            long long* num_batches_tracked, float momentum, float eps, float* scale, float* shift, float* save_mean,
                            float* save_invstd, void* stream);
int runet_bn_finalize(const float* mean_nc, const float* m2_nc, int n_img, int c, long hw, const float* gamma, const float* beta,
                      float* run_mean, float* run_var, long long* num_batches_tracked, float momentum, float eps, int training,
                      float* scale, float* shift, float* save_mean, float* save_invstd, void* stream);

/* runet_chan_stats + runet_bn_finalize(training) without the per-image outputs, in two launches instead of three (the forward of
 * nn.BatchNorm2d in training mode, Main_Final.py:158,160, wherever no per-image statistics are needed): partials per chunk, then one
 * kernel that Chan-combines all of a channel's partials and derives scale / shift / saved and running statistics. */
int runet_bn_stats(const float* x, int ld, int n_img, int hw, int c, float* workspace, const float* gamma, const float* beta,
                   float* run_mean, float* run_var, long long* num_batches_tracked, float momentum, float eps, float* scale,
                   float* shift, float* save_mean, float* save_invstd, void* stream);

/* y = [relu](x*scale[c] + shift[c]) [* mask_nc[n, c]]   (mask = Dropout2d keep-mask already divided by 1-p, or NULL) */
int runet_bn_apply(const float* x, int ldx, float* y, int ldy, long pixels, int hw, int c, const float* scale, const float* shift,
                   const float* mask_nc, int relu, void* stream);

/* g = dy, or dy*mask_nc[n,c]*(act > 0) when act != NULL (act = saved output of relu/dropout), or - relu_scale/relu_shift given, act NULL -
 * dy*mask_nc[n,c]*(x*relu_scale[c] + relu_shift[c] > 0): the forward's affine recomputed from x, one tensor less to read.  Both forms give the same bits: where mask_nc[n,c] is 0, g is +0 in either.
 * sums[0:c] = sum g*xhat (= dgamma), sums[c:2c] = sum g (= dbeta): the order of (weight, bias). */
int runet_bn_bwd_reduce(const float* dy, int lddy, const float* x, int ldx, const float* act, int ldact, int n_img, int hw, int c,
                        const float* mean, const float* invstd, const float* mask_nc, float* workspace, float* sums, const float* relu_scale,
                        const float* relu_shift, void* stream);
/* dx = scale*(g - sums[C+c]/M - xhat*sums[c]/M), M = m_total if > 0 else pixels (SyncBN: sums all-reduced, M = global count);
 * relu_shift (act NULL): g as above with relu_scale = scale */
int runet_bn_bwd_apply(const float* dy, int lddy, const float* x, int ldx, const float* act, int ldact, float* dx, int lddx,
                       long pixels, int hw, int c, const float* mean, const float* invstd, const float* scale, const float* sums,
                       const float* mask_nc, long m_total, const float* relu_shift, void* stream);
/* out[c] (=|+=) sum over pixels of x[p, c]  (bias gradients) */
int runet_chan_sum(const float* x, int ld, long pixels, int c, float* workspace, float* out, int accumulate, void* stream);

/* ---- ChannelAttention / SpatialAttention / ResidualBlock tail (Main_Final.py:82-117, 186-194) ----
 * w0p = ca.fc.0 weight as [C][Cr], w2p = ca.fc.2 weight as [Cr][C], wp = sa.conv1 weight as [7][7][2]. */
int runet_ca_coeff(const float* mean_nc, const float* max_nc, const float* min_nc, const int* imax_nc, const int* imin_nc,
                   const float* s2, const float* h2, const float* w0p, const float* w2p, int n_img, int c, int cr, float* A, float* B,
                   float* ca, float* avg, float* mx, int* idx, float* tval, void* stream);
int runet_sa_reduce(const float* t2, int ld, const float* A, const float* B, long pixels, int hw, int c, float* smap, int* amax,
                    void* stream);
int runet_sa_conv7(const float* smap, const float* wp, float* sa, int n_img, int h, int w, void* stream);
/* out = relu((t2*A[n,c]+B[n,c])*sa[p] + res),  res = r*rs[c]+rh[c]  (rs == NULL: res = r, identity shortcut) */
int runet_rb_out(const float* t2, int ld, const float* A, const float* B, const float* sa, const float* r, int ldr, const float* rs,
                 const float* rh, float* out, int ldo, long pixels, int hw, int c, void* stream);
/* dv = dout * (out > 0) (out NULL: dv = dout, no ReLU behind the attention), dq[p] = (sum_c dv*u) * sa*(1-sa) with u = t2*A+B */
int runet_rb_bwd1(const float* dout, int lddo, const float* out, int ldo, const float* t2, int ld, const float* A, const float* B,
                  const float* sa, float* dv, int lddv, float* dq, long pixels, int hw, int c, void* stream);
/* The block's edges folded into its tail (the encoder blocks of Main_Final.py:235-249 feed nn.MaxPool2d(2); :194 is the ReLU):
 * runet_rb_out_ex = runet_rb_out, plus
 *   relu_bits [pixels][c/4] (or NULL): one byte per 4 channels, bit e set when out[p, 4j+e] > 0 - runet_rb_bwd1_ex's ReLU mask;
 *   pooled [n, h/2, w/2, c] (pixel stride ldp) + pool_idx (or both NULL): runet_maxpool2_fwd(out), same values and winner bytes
 *   (dense, c per pooled pixel, byte k = dy*2 + dx of the first maximum).
 * runet_rb_bwd1_ex = runet_rb_bwd1 on dout + runet_maxpool2_bwd(dpool, pool_idx) (dpool NULL: on dout alone; dout is not modified),
 *   the ReLU mask from relu_bits when given, else from out (both NULL: no ReLU). */
int runet_rb_out_ex(const float* t2, int ld, const float* A, const float* B, const float* sa, const float* r, int ldr, const float* rs,
                    const float* rh, float* out, int ldo, unsigned char* relu_bits, float* pooled, int ldp, unsigned char* pool_idx, int n_img,
                    int h, int w, int c, void* stream);
int runet_rb_bwd1_ex(const float* dout, int lddo, const float* dpool, int ldp, const unsigned char* pool_idx, const float* out, int ldo,
                     const unsigned char* relu_bits, const float* t2, int ld, const float* A, const float* B, const float* sa, float* dv,
                     int lddv, float* dq, int n_img, int h, int w, int c, void* stream);
/* The 64 -> 1 head (outc below) folded into the tail of the block in front of it; bit for bit what the separate launches give.
 * runet_rb_out_head = runet_rb_out_ex(no pool) + runet_outc_fwd(out, hw [c], hb [1], logit (or NULL), prob) taken from the values it
 *   stores, without the re-read of `out` (which is still written).  c == 64 only: runet_rb_out_head_supported.
 * runet_rb_bwd1_rank1 = runet_rb_bwd1_ex(no pool, mask from relu_bits) on dout[p][c] = hw[c] * dl[p], the head's data gradient, formed in
 *   the load from dl [pixels] (runet_outc_bwd_dl) instead of being written and read back as a tensor. */
int runet_rb_out_head_supported(int c);
int runet_rb_out_head(const float* t2, int ld, const float* A, const float* B, const float* sa, const float* r, int ldr, const float* rs,
                      const float* rh, float* out, int ldo, unsigned char* relu_bits, const float* hw, const float* hb, float* logit,
                      float* prob, int n_img, int h, int w, int c, void* stream);
int runet_rb_bwd1_rank1(const float* dl, const float* hw, const unsigned char* relu_bits, const float* t2, int ld, const float* A,
                        const float* B, const float* sa, float* dv, int lddv, float* dq, int n_img, int h, int w, int c, void* stream);
long runet_sa_conv7_bwd_workspace_floats(int n_img, int h, int w);
int runet_sa_conv7_bwd(const float* smap, const float* dq, const float* wp, float* dsm, float* dwp, float* workspace, int n_img, int h,
                       int w, void* stream);
int runet_rb_bwd2(const float* dv, int lddv, const float* t2, int ld, const float* sa, const float* dsm, const int* amax, int n_img,
                  int hw, int c, float* workspace, float* sdu, float* sdut, void* stream);
/* runet_rb_bwd2 that also leaves the LOCAL BatchNorm-backward sums of the block's shortcut BatchNorm (Main_Final.py:173) behind: dv is that
 * BatchNorm's incoming gradient and r its input; sums_s [2c] = (sum dv * rhat | sum dv), what runet_bn_bwd_reduce(dv, r) would compute */
long runet_rb_bwd2_bn_workspace_floats(int n_img, int hw, int c);
int runet_rb_bwd2_bn(const float* dv, int lddv, const float* t2, int ld, const float* sa, const float* dsm, const int* amax, const float* r, int ldr,
                     const float* mean_s, const float* invstd_s, int n_img, int hw, int c, float* workspace, long workspace_floats, float* sdu,
                     float* sdut, float* sums_s, void* stream);
long runet_ca_bwd_workspace_floats(int n_img, int c, int cr);
int runet_ca_bwd(const float* sdu, const float* sdut, const float* s2, const float* h2, const float* ca, const float* avg, const float* mx,
                 const float* w0p, const float* w2p, const float* mean_nc, const float* tval, const float* mean2, const float* invstd2,
                 int n_img, int c, int cr, float* workspace, float* davg, float* dmx, float* sums2, float* dw0p, float* dw2p, void* stream);
int runet_rb_bwd3(const float* dv, int lddv, const float* t2, int ld, const float* sa, const float* dsm, const int* amax, const float* ca,
                  const float* davg, const float* dmx, const int* idx, const float* mean2, const float* invstd2, const float* s2,
                  const float* sums2, float* dt2, int lddt, long pixels, int hw, int c, long m_total, void* stream);
/* runet_rb_bwd3 of a block with a convolution shortcut (Main_Final.py:170-174) that also applies the shortcut BatchNorm's backward: dv, that
 * BatchNorm's incoming gradient, is overwritten with dr = runet_bn_bwd_apply(dv, r, mean_s, invstd_s, scale_s, sums_s, m_total_s) (no
 * activation, no mask); sums_s as runet_bn_bwd_reduce(dv, r) left them (or all-reduced, or zeros in eval mode). */
int runet_rb_bwd3_sc(float* dv, int lddv, const float* t2, int ld, const float* sa, const float* dsm, const int* amax, const float* ca,
                     const float* davg, const float* dmx, const int* idx, const float* mean2, const float* invstd2, const float* s2,
                     const float* sums2, float* dt2, int lddt, const float* r, int ldr, const float* mean_s, const float* invstd_s,
                     const float* scale_s, const float* sums_s, long m_total_s, long pixels, int hw, int c, long m_total, void* stream);

/* ---- AttentionGate (Main_Final.py:120-148): psi conv (F_int -> 1) and the gating multiply ---- */
int runet_ag_psi(const float* g1, int ldg, const float* x1, int ldx, const float* sg, const float* hg, const float* sx, const float* hx,
                 const float* wpsi, const float* bpsi, float* s, long pixels, int f, void* stream);
int runet_ag_out(const float* xs, int ldx, const float* s, const float* sp, const float* hp, float* out, int ldo, long pixels, int c,
                 void* stream);
int runet_ag_bwd1(const float* datt, int ldd, const float* xs, int ldx, const float* s, const float* sp, const float* hp, float* dxs,
                  int lddx, float* dsbn, long pixels, int c, void* stream);
/* dwpsi_db: [f] weight gradient followed by the bias gradient at index f */
int runet_ag_bwd2(const float* ds, const float* g1, int ldg, const float* x1, int ldx, const float* sg, const float* hg, const float* sx,
                  const float* hx, const float* wpsi, float* dpre, int ldp, float* workspace, float* dwpsi_db, long pixels, int f,
                  void* stream);
/* runet_ag_bwd2 that also leaves the LOCAL BatchNorm-backward sums of the gate's two BatchNorms (W_g.1, W_x.1: Main_Final.py:127,132) behind -
 * sums_g / sums_x [2f] = (sum dpre * xhat | sum dpre), what runet_bn_bwd_reduce would compute from (dpre, g1) and (dpre, x1) */
long runet_ag_bwd2_bn_workspace_floats(long pixels, int f);
int runet_ag_bwd2_bn(const float* ds, const float* g1, int ldg, const float* x1, int ldx, const float* sg, const float* hg, const float* sx,
                     const float* hx, const float* wpsi, const float* mean_g, const float* invstd_g, const float* mean_x, const float* invstd_x,
                     float* dpre, int ldp, float* workspace, long workspace_floats, float* dwpsi_db, float* sums_g, float* sums_x, long pixels, int f,
                     void* stream);

/* ---- outc: Conv2d(C, 1, 1) + Sigmoid (Main_Final.py:274-277) ----
 * runet_outc_bwd: prob NULL = `dprob` is already the logit's gradient (a head whose sigmoid sits behind an upsampling: runet_up_sigmoid_bwd) */
int runet_outc_fwd(const float* x, int ld, const float* w, const float* b, float* logit, float* prob, long pixels, int c, void* stream);
int runet_outc_bwd(const float* dprob, const float* prob, const float* x, int ld, const float* w, float* dx, int lddx, float* workspace,
                   float* dw_db, long pixels, int c, void* stream);
/* runet_outc_bwd without dx: the same dw_db, and dl [pixels] = dprob*prob*(1-prob) (prob NULL: dprob) for runet_rb_bwd1_rank1 */
int runet_outc_bwd_dl(const float* dprob, const float* prob, const float* x, int ld, float* dl, float* workspace, float* dw_db,
                      long pixels, int c, void* stream);

/* ---- MaxPool2d(2) (Main_Final.py:235,239,243,249); idx: one byte per output element ---- */
int runet_maxpool2_fwd(const float* x, int ldx, float* y, int ldy, unsigned char* idx, int n_img, int h, int w, int c, void* stream);
int runet_maxpool2_bwd(const float* dy, int lddy, const unsigned char* idx, float* dx, int lddx, int n_img, int h, int w, int c,
                       int accumulate, void* stream);
/* strided [N,C,H,W] -> dense NHWC with channels zero-padded to c_pad (module entry: Main_Final.py:290 input x) */
int runet_to_nhwc_pad(const float* x, long sn, long sc, long sh, long sw, float* y, int n_img, int c, int h, int w, int c_pad, void* stream);

/* ---- nn.BCELoss() mean (Main_Final.py:551,580): logs clamped at -100; backward (p-y)/max(p(1-p),1e-12)/n * grad_out[0] ---- */
int runet_bce_fwd(const float* prob, const float* target, long n, double* workspace1024, float* loss, void* stream);
int runet_bce_bwd(const float* prob, const float* target, const float* grad_out, float* dprob, long n, void* stream);

/* ---- torch.optim.Adam(lr, weight_decay) (Main_Final.py:552,582), all tensors in one launch ----
 * table: device int64 [5][n_tensors] = param, grad, exp_avg, exp_avg_sq pointers, element counts;
 * chunks: device int32 [n_chunks][2] = (tensor index, chunk index), chunk = runet_adam_chunk_elems() elements.
 * grad_scale multiplies the gradient first (1/world_size after a sum all-reduce, 1/loss_scale under loss scaling).
 * skip_flag (may be NULL): device int; non-zero -> the whole update is skipped (runet_nonfinite_flag found Inf / NaN gradients). */
int runet_adam_chunk_elems(void);
int runet_adam_multi(const long long* table, int n_tensors, const int* chunks, int n_chunks, float lr, float beta1, float beta2, float eps,
                     float weight_decay, int step, float grad_scale, const int* skip_flag, void* stream);

/* hipGraph-capturable form: hyper = device float[6] {lr, beta1, beta2, eps, weight_decay, grad_scale}; *step_dev is incremented on the
 * device and then used for the bias corrections, so one captured launch serves every step and every learning rate. */
int runet_adam_multi_dev(const long long* table, int n_tensors, const int* chunks, int n_chunks, const float* hyper, int* step_dev,
                         const int* skip_flag, void* stream);
/* loss scaling: flag2[0] = 1 iff buf[0:n] holds an Inf / NaN (reset by this call), flag2[1] += flag2[0] (running count of skipped steps) */
int runet_nonfinite_flag(const float* buf, long n, int* flag2, void* stream);
/* stream `waiter` waits for everything enqueued on stream `waited` so far (event record + stream wait on a pooled event): host-side helper
 * of the weight-gradient side stream (the all-reduce / backward overlap of Main_Final.py:581's loss.backward()). */
int runet_stream_wait(void* waiter, void* waited);


/* ---- ModelEvaluator.calculate_metrics counts (Main_Final.py:519-547): counts[n] = {tp, pred>thr, target!=0, agree} ---- */
int runet_seg_counts(const float* pred, const float* target, long long* counts, int n_img, long per_img, float threshold, void* stream);

/* ---- batched plain GEMMs (fp32 MFMA, LDS-tiled; the position-GEMMs of the F(4x4,3x3) path) ----
 * runet_gemm_batched:    C[z][rows][n] = A[z][rows][k] . B[z][k][n]   (row strides lda / n / ldc, batch strides in floats)
 * runet_gemm_tn_batched: C[split][z][k][n] = sum over rows of split of A[z][row][k] * B[z][row][n];  splits = ceil(rows / rows_per_split) */
int runet_gemm_batched(const float* a, int lda, long stride_a, const float* b, long stride_b, float* c, int ldc, long stride_c, int batch, int rows,
                       int k, int n, void* stream);
int runet_gemm_tn_batched(const float* a, int lda, long stride_a, const float* b, int ldb, long stride_b, float* c, int batch, int rows, int k, int n,
                          int rows_per_split, void* stream);
/* name of the device kernel runet_gemm_batched launches for this shape (128x128 LDS-ring kernel, or 128x64 tiles where those would
 * fill the 256 CUs unevenly) - for matching live timings with rocprofv3 rows */
const char* runet_gemm_batched_kernel_name(int batch, int rows, int k, int n);

/* ---- the same GEMMs in fp32 on the BF16 matrix cores: exact three-way operand splitting, six bf16 MFMAs per fp32 product ("bf16x6") ----
 * The f32-input MFMA runs at 1/16 of the bf16 MFMA rate on gfx950.  x = h + m + l with three bf16 values holds exactly for every finite fp32 x,
 * FLT_MAX included (h from x clamped to +-bf16-max; Inf and NaN operands give non-finite results: DESIGN.md 3.0, C1 - C4);
 * six of the nine cross products are kept (the three dropped are <= 2^-23 of the product, the size of one fp32 rounding), all accumulate in
 * fp32: an fp32-accurate GEMM at 6/16 of the matrix time (csrc/gemm_split.hip; measured against float64 in tests/test_gpu_conv.py).
 * These serve the same role as runet_gemm_batched / runet_gemm_tn_batched (the position-GEMMs of nn.Conv2d 3x3, Main_Final.py:157,159).
 * runet_gemm_x3_pack: B fp32 [z][k][n] (the weights side: once per optimizer step) -> packed split planes [z][3][k/8][n][8] bf16,
 *   runet_gemm_x3_pack_elems(batch, k, n) 2-byte elements.  runet_gemm_x3_batched: C[z][rows][n] = A[z][rows][k] . B[z] with A fp32 split on
 *   the fly (k % 16 == 0).  runet_gemm_x3_tn_batched: as runet_gemm_tn_batched, both operands fp32 (rows, rows_per_split multiples of 16). */
int runet_gemm_x3_supported(int rows, int k, int n);
long runet_gemm_x3_pack_elems(int batch, int k, int n);
int runet_gemm_x3_pack(const float* b, long stride_b, void* packed, int batch, int k, int n, void* stream);
int runet_gemm_x3_batched(const float* a, int lda, long stride_a, const void* packed_b, float* c, int ldc, long stride_c, int batch, int rows,
                          int k, int n, void* stream);
int runet_gemm_x3_tn_batched(const float* a, int lda, long stride_a, const float* b, int ldb, long stride_b, float* c, int batch, int rows, int k,
                             int n, int rows_per_split, void* stream);
const char* runet_gemm_x3_kernel_name(int batch, int rows, int k, int n);
/* weight gradient of ConvTranspose2d(k2, s2) (Main_Final.py:261-270) on the same TN kernel: x [n_img,h,w,cin], dy [n_img,2h,2w,cout] ->
 * c [splits][2][2][cin][cout] (sum the splits in order: runet_conv_wgrad does); w % 16 == 0, rows_per_split % 16 == 0 */
int runet_gemm_x3_tn_convt(const float* x, int ldx, const float* dy, int ldy, float* c, int n_img, int h, int w, int cin, int cout,
                           int rows_per_split, void* stream);

/* ---- nn.Conv2d(k=1) (Main_Final.py:126,131,172,205) and nn.ConvTranspose2d(k=2, s=2) (:261-270), forward and data gradient, by the same
 * split-operand scheme (csrc/conv_x3.hip): same modes and argument meaning as runet_conv_igemm (RUNET_CONV_FWD, RUNET_CONV_DGRAD,
 * RUNET_CONVT_FWD, RUNET_CONVT_DGRAD; cin = channels READ in that mode, cout = channels WRITTEN; h, w = the image the 1x1 convolution runs
 * over, for the transposed modes the low-resolution side), but the weight comes pre-split: runet_conv_x3_pack turns the module's forward
 * weight (HWIO: [cin][cout], transposed [2][2][Ci][Co]; the data-gradient modes read it transposed) into runet_conv_x3_pack_elems 2-byte
 * elements, once per optimizer step.  cin % 16 == 0, cout % 4 == 0, ldx % 4 == 0, x 16-byte aligned. */
int runet_conv_x3_supported(int cin, int cout, int mode);
long runet_conv_x3_pack_elems(int cin, int cout, int mode);
int runet_conv_x3_pack(const float* w, void* packed, int cin, int cout, int mode, void* stream);
int runet_conv_x3(const float* x, int ldx, const void* wpacked, const float* bias, float* y, int ldy, int n_img, int h, int w, int cin, int cout,
                  int mode, int accumulate, void* stream);
const char* runet_conv_x3_kernel_name(int n_img, int h, int w, int cout, int mode);

/* ---- the narrow nn.Conv2d(k=1) layers (Main_Final.py:126,131,172), forward and data gradient, as a streaming kernel with the weight
 * resident in LDS (csrc/conv1x1_stream.hip): persistent blocks, one weight load per block, no block barrier in the pixel loop, the next
 * tile's loads in flight across the current tile's MFMAs.  Modes RUNET_CONV_FWD (w [cin][cout]) and RUNET_CONV_DGRAD (w = the module's
 * forward weight [cout][cin], read transposed) with runet_conv_igemm's argument meaning; cin % 16 == 0, cout % 4 == 0, both <= 128,
 * ldx / ldy % 4 == 0, pointers 16-byte aligned.  y has the bits runet_conv_igemm gives (same fp32 MFMA chain per element, acc + bias + old).
 * runet_conv1x1_stream_blocks: the number of persistent blocks of a launch (from the CU count; RUNET_CONV1X1_STREAM_BLOCKS, read at
 * call time, forces it: measurement knob).  runet_conv1x1_stream_kernel_name: the instantiation's name as rocprofv3 prints it. */
int runet_conv1x1_stream_supported(int cin, int cout, int mode);
int runet_conv1x1_stream_blocks(int n_img, int h, int w, int cin, int cout);
int runet_conv1x1_stream(const float* x, int ldx, const float* w, const float* bias, float* y, int ldy, int n_img, int h, int w_, int cin,
                         int cout, int mode, int accumulate, void* stream);
const char* runet_conv1x1_stream_kernel_name(int cin, int cout, int accumulate);
/* weight gradient of the same layers (Main_Final.py:581 loss.backward()): dw[cin][cout] = sum over pixels of x (x) dy, the pixel as the MFMA
 * contraction, every wave streaming a contiguous pixel range with the whole result in registers; one slab per block in `workspace`
 * (>= runet_conv1x1_wgrad_stream_workspace_floats floats), summed in a fixed order.  cin, cout in {32, 64, 128}, not both 128.  The slab
 * count depends on the pixel count alone (runet_conv1x1_wgrad_stream_slabs: ceil(pixels / 256), at most 256), so the result is bitwise
 * reproducible from run to run and on every device. */
int runet_conv1x1_wgrad_stream_supported(int cin, int cout);
int runet_conv1x1_wgrad_stream_slabs(int n_img, int h, int w);
long runet_conv1x1_wgrad_stream_workspace_floats(int n_img, int h, int w, int cin, int cout);
int runet_conv1x1_wgrad_stream(const float* x, int ldx, const float* dy, int ldy, float* dw, float* workspace, long workspace_floats,
                               int n_img, int h, int w_, int cin, int cout, void* stream);

/* ---- every derived weight of a step in one launch (csrc/derive_multi.hip).  The split-operand kernels read their weights as bf16 planes made
 * by runet_wino4_weights_x3 / runet_wino_weights_x3 / runet_conv_x3_pack once per optimizer step (the reference has no such step: its weights
 * are read as they are, Main_Final.py:123-134, 261-270); these three calls batch them: fill a host table with runet_derive_desc (same arguments as
 * the per-tensor call of that kind; returns the entry's block count, < 0 on bad arguments), copy it to the device, launch runet_derive_multi.
 * Results are bit-identical to the per-tensor calls. */
enum { RUNET_DERIVE_WINO4 = 0, RUNET_DERIVE_WINO2 = 1, RUNET_DERIVE_PACK = 2 };
int runet_derive_desc_bytes(void);
int runet_derive_desc(void* host_table, int index, int kind, const float* w, void* dst, int cin, int cout, int mode, int first_block);
int runet_derive_multi(const void* table, int n_desc, int total_blocks, void* stream);
/* the 1x1 modes with the BatchNorm statistics of the output taken in the epilogue: stats [runet_conv_x3_stats_parts(n_img, h, w)][cout][3] */
int runet_conv_x3_stats_parts(int n_img, int h, int w);
int runet_conv_x3_stats(const float* x, int ldx, const void* wpacked, const float* bias, float* y, int ldy, int n_img, int h, int w, int cin, int cout,
                        int mode, int accumulate, float* stats, void* stream);

/* ---- Winograd F(4x4,3x3), unfused, for the deep 3x3 convolutions (Main_Final.py:157,159 at >= 256 channels) and their autograd ----
 * U [36][K][N] from runet_wino4_weights (dgrad != 0: rotated filter, K = cout, N = cin).  conv: x [n,h,w,K] -> y [n,h,w,N] ('same'), H, W % 4 == 0.
 * dil >= 1 (padding = dil: the bottleneck's DilatedBlock, Main_Final.py:207-208): the dilated convolution is run as dil*dil independent
 * dilation-1 convolutions over the (h/dil) x (w/dil) sub-images of every image, so (h/dil) % 4 == 0 and (w/dil) % 4 == 0 are required.
 * workspace: runet_wino4_workspace_floats / runet_wino4_wgrad_workspace_floats floats, 16-byte aligned. */
int runet_wino4_supported(int h, int w, int k, int n);
long runet_wino4_workspace_floats(int n_img, int h, int w, int k, int n);
int runet_wino4_weights(const float* w_hwio, float* U, int cin, int cout, int dgrad, void* stream);
int runet_wino4_conv(const float* x, int ldx, const float* U, const float* bias, float* y, int ldy, int n_img, int h, int w, int k, int n,
                     int dil, int accumulate, float* workspace, long workspace_floats, void* stream);
/* runet_wino4_weights + runet_gemm_x3_pack in one pass: the filter transform written straight into the split planes (36 matrices [k][n] ->
 * [36][3][k/8][n][8] bf16, runet_gemm_x3_pack_elems(36, k, n) elements); k (cin, or cout when dgrad != 0) a multiple of 8 */
int runet_wino4_weights_x3(const float* w_hwio, void* Upacked, int cin, int cout, int dgrad, void* stream);
/* runet_wino4_conv with the position-GEMMs on the bf16 matrix cores (split operands, fp32-accurate): Upacked = runet_gemm_x3_pack of U; k % 16 == 0 */
int runet_wino4_conv_x3(const float* x, int ldx, const void* Upacked, const float* bias, float* y, int ldy, int n_img, int h, int w, int k, int n,
                        int dil, int accumulate, float* workspace, long workspace_floats, void* stream);
/* the stages of the two composites below, one kernel each (T = n_img*(h/4)*(w/4) tiles):
 *   runet_wino4_input  mode 0: V[36][T][c] = B^T d B (6x6 patches of src, stride 4, 1-pixel halo); mode 1: Z[36][T][c] = A dY A^T (4x4 tiles)
 *   runet_gemm_batched / runet_gemm_tn_batched: the 36 position-GEMMs
 *   runet_wino4_output: y = A^T M A (+bias, +y);  runet_wino4_wgrad_output: dw[3][3][cin][cout] = G^T (sum_splits dU[split][36][cin][cout]) G */
int runet_wino4_input(const float* src, int ld, int c, int n_img, int h, int w, int dil, int mode, float* V, void* stream);
/* The same transforms with their input's elementwise producer folded into the loads (the tensor between the two is never written; results
 * bit-identical to the two-step forms).  runet_wino4_input_act: mode 0 of a1 = runet_bn_apply(t, scale, shift, factor_nc, relu = 1), i.e. the
 * BatchNorm + ReLU + Dropout2d in front of a ResidualBlock's conv2 (Main_Final.py:157-160).  runet_wino4_input_bn_bwd: mode 1 of
 * dx = runet_bn_bwd_apply(dy, x, ..., relu_shift = shift), i.e. autograd's backward of that BatchNorm + ReLU feeding conv1's gradients; sums as
 * runet_bn_bwd_reduce leaves them, m_total 0 = the tensor's own pixel count. */
int runet_wino4_input_act(const float* t, int ld, int c, int n_img, int h, int w, int dil, const float* scale, const float* shift,
                          const float* factor_nc, float* V, void* stream);
int runet_wino4_input_bn_bwd(const float* dy, int lddy, const float* x, int ldx, int c, int n_img, int h, int w, int dil, const float* mean,
                             const float* invstd, const float* scale, const float* shift, const float* sums, const float* factor_nc,
                             long m_total, float* Z, void* stream);
int runet_wino4_output(const float* M, int n, int n_img, int h, int w, int dil, const float* bias, float* y, int ldy, int accumulate, void* stream);
/* runet_wino4_output (dil = 1) that also leaves the BatchNorm statistics partials of y behind for runet_bn_stats_finalize: stats
 * [runet_wino4_output_stats_parts(...)][n][3] = (count, mean, M2); _parts returns 0 where the kernel cannot take them (n / 2 not a power of two, dil != 1). */
int runet_wino4_output_stats_parts(int n_img, int h, int w, int n, int dil);
int runet_wino4_output_stats(const float* M, int n, int n_img, int h, int w, const float* bias, float* y, int ldy, int accumulate, float* stats, void* stream);
/* The data gradient as the ADJOINT of the forward algorithm: Z = A dy A^T (runet_wino4_input mode 1 - the weight gradient's transform, shared),
 * M' = Z . U^T by the position GEMMs (runet_wino4_weights_x3 with dgrad = 2: the forward's U transposed, not rotated), and this gather-form
 * output transform dx = overlap-add of B M' B^T: one pass over dy and one filter transform less than the convolution form per layer. */
int runet_wino4_output_adj(const float* M, int n, int n_img, int h, int w, int dil, float* y, int ldy, int accumulate, void* stream);
int runet_wino4_wgrad_output(const float* dU, int splits, int cin, int cout, float* dw, void* stream);
int runet_wino4_wgrad_rows_per_split(int n_img, int h, int w, int cin, int cout);
long runet_wino4_wgrad_workspace_floats(int n_img, int h, int w, int cin, int cout);
int runet_wino4_wgrad(const float* x, int ldx, const float* dy, int ldy, float* dw, float* workspace, long workspace_floats, int n_img, int h, int w,
                      int cin, int cout, int dil, void* stream);

/* ---- the RGB stem (Main_Final.py:157,172 with in_channels = 3; `inc` :235): 1..3 real input channels in an NHWC tensor padded to 4 ----
 * runet_stem_conv: y3 = conv3x3(x, w3 [3][3][cin_w][cout], padding 1) and, if w1 != NULL, y1 = conv1x1(x, w1 [cin_w][cout]) (the first
 * ResidualBlock's shortcut) in ONE launch: x is read once, both filters form one register-resident B matrix.  No bias (the block's
 * convolutions have none).  runet_stem_wgrad: dw [k][k][cin_w][cout] of either convolution (ksize 3 or 1) with the pixels as the MFMA
 * contraction; workspace: runet_stem_wgrad_workspace_floats floats.  cout 32 or 64 (runet_stem_supported). */
int runet_stem_supported(int cin_w, int cout);
int runet_stem_conv(const float* x, int ldx, const float* w3, const float* w1, float* y3, int ldy3, float* y1, int ldy1, int n_img,
                    int h, int w, int cin_w, int cout, void* stream);
/* runet_stem_conv that also leaves the BatchNorm statistics partials of y3 (and y1) behind for runet_bn_stats_finalize:
 * stats3 / stats1 [runet_stem_conv_stats_parts(n_img, h, w)][cout][3] = (count, mean, M2) per 8 x 32 pixel tile */
int runet_stem_conv_stats_parts(int n_img, int h, int w);
int runet_stem_conv_stats(const float* x, int ldx, const float* w3, const float* w1, float* y3, int ldy3, float* y1, int ldy1, int n_img,
                          int h, int w, int cin_w, int cout, float* stats3, float* stats1, void* stream);
long runet_stem_wgrad_workspace_floats(int n_img, int h, int w, int cin_w, int cout, int ksize);
int runet_stem_wgrad(const float* x, int ldx, const float* dy, int ldy, float* dw, float* workspace, long workspace_floats, int n_img,
                     int h, int w, int cin_w, int cout, int ksize, void* stream);

/* ---- DeepLabV3+ baseline (Main_Final.py:325-433): the same implicit-GEMM kernels with general geometry ----
 * runet_conv2d_general: Conv2d(kh x kw <= 8x8, stride 1..8, padding, dilation).  mode RUNET_CONV_FWD: x [n,hin,win,cin] -> y [n,ho,wo,cout],
 * (kernel = stride, no padding, hin = ho * stride: the data gradient takes the one live tap per pixel, s^2 GEMMs + a permutation)
 * w [kh,kw,cin_w,cout];  mode RUNET_CONV_DGRAD: x := dy [n,ho,wo,cin(=conv Cout)] -> y := dx [n,hin,win,cout(=conv Cin)], w [kh,kw,cout,cin].
 * runet_convt4_igemm: ConvTranspose2d(k4, s2, p1), w [4,4,cin,cout]; RUNET_CONVT_FWD x [n,h,w,cin] -> y [n,2h,2w,cout];
 * RUNET_CONVT_DGRAD x := dy [n,2h,2w,cin(=Cout)] -> y := dx [n,h,w,cout(=Cin)].
 * runet_conv_wgrad_general: dw of either (transposed4 != 0: the k4 transposed conv, x [n,hin,win,cin], dy [n,2hin,2win,cout]). */
int runet_conv2d_general(const float* x, int ldx, const float* w, const float* bias, float* y, int ldy, int n_img, int hin, int win, int cin,
                         int cin_w, int cout, int kh, int kw, int stride, int pad, int dil, int mode, int accumulate, void* stream);
int runet_convt4_igemm(const float* x, int ldx, const float* w, const float* bias, float* y, int ldy, int n_img, int h, int w_, int cin, int cout,
                       int mode, int accumulate, void* stream);
long runet_conv_wgrad_general_workspace_floats(int pixels, int cin_w, int cout, int kh, int kw);
int runet_conv_wgrad_general(const float* x, int ldx, const float* dy, int ldy, float* dw, float* workspace, long workspace_floats, int n_img,
                             int hin, int win, int cin, int cin_w, int cout, int kh, int kw, int stride, int pad, int dil, int transposed4,
                             void* stream);
/* MaxPool2d(3, stride 2, padding 1) (Main_Final.py:369); idx: one byte per output element (window position of the first maximum) */
int runet_maxpool3s2_fwd(const float* x, int ldx, float* y, int ldy, unsigned char* idx, int n_img, int h, int w, int c, void* stream);
int runet_maxpool3s2_bwd(const float* dy, int lddy, const unsigned char* idx, float* dx, int lddx, int n_img, int h, int w, int c, void* stream);
/* dst[i] += src[i] (dense buffers): joins the ASPP image-pooling gradient with the other four branches' */
int runet_add_inplace(float* dst, const float* src, long n, void* stream);
/* y[n, p, 0:c] = v[n, 0:c]: bilinear upsampling of the ASPP image-pooling branch's 1x1 map (Main_Final.py:350-352) */
int runet_broadcast_nc(const float* v_nc, float* y, int ldy, int n_img, int hw, int c, void* stream);
/* decoder head Conv2d(c, 1, 3, padding 1) + sigmoid (Main_Final.py:414,433); w [3,3,c] ; dw_db = [9*c] weight gradient then the bias gradient */
int runet_head3x3_fwd(const float* x, int ld, const float* w, const float* b, float* prob, int n_img, int h, int w_, int c, void* stream);
long runet_head3x3_bwd_workspace_floats(int n_img, int h, int w_, int c);
int runet_head3x3_bwd(const float* dprob, const float* prob, const float* x, int ld, const float* w, float* dx, int lddx, float* workspace,
                      float* dw_db, int n_img, int h, int w_, int c, void* stream);


/* ---- bf16-operand convolutions (BASELINE.json configs 3 and 5: "bf16" / reduced precision; the reference itself is fp32 only, so the
 *      oracle for this path is the fp32 step and the tolerance is stated in tests/test_gpu_bf16.py) ----
 * Only the two operands of each convolution's multiply-adds are rounded to bf16 (round-to-nearest-even) on their way into LDS;
 * accumulation, activations in HBM, master weights, BatchNorm, attention, loss and Adam stay fp32.
 * runet_bf16_pack_weights: HWIO fp32 w[taps][cin][cout] -> packed bf16 [taps][K/8][N][8] (K padded to a multiple of 8 with zeros);
 *   transpose == 0: K = cin, N = cout (forward, k2-s2 transposed forward);  transpose != 0: K = cout, N = cin (data gradients).
 *   `packed` holds runet_bf16_pack_elems(taps, K, N) 16-bit elements.
 * runet_conv_igemm_bf16: same modes / geometry as runet_conv_igemm (cin_w == cin), weights from runet_bf16_pack_weights.
 * runet_conv_wgrad_bf16: same contract as runet_conv_wgrad (cin_w == cin; dil only for 3x3).
 * The *_fp16 entry points are the same kernels with IEEE half operands (BASELINE config 5 names fp16; csrc/conv_fp16.hip); train with a
 * loss scale (runet_nonfinite_flag + the skip_flag of the fused Adam). */
long runet_bf16_pack_elems(int taps, int k, int n);
int runet_bf16_pack_weights(const float* w_hwio, void* packed, int taps, int cin, int cout, int transpose, void* stream);
int runet_conv_igemm_bf16(const float* x, int ldx, const void* wpacked, const float* bias, float* y, int ldy, int n_img, int h, int w_,
                          int cin, int cout, int kh, int kw, int dil, int mode, int accumulate, void* stream);
long runet_conv_wgrad_bf16_workspace_floats(int n_img, int h, int w_, int cin, int cout, int kh, int kw, int dil, int transposed);
int runet_conv_wgrad_bf16(const float* x, int ldx, const float* dy, int ldy, float* dw, float* workspace, long workspace_floats,
                          int n_img, int h, int w_, int cin, int cout, int kh, int kw, int dil, int transposed, void* stream);

long runet_fp16_pack_elems(int taps, int k, int n);
int runet_fp16_pack_weights(const float* w_hwio, void* packed, int taps, int cin, int cout, int transpose, void* stream);
int runet_conv_igemm_fp16(const float* x, int ldx, const void* wpacked, const float* bias, float* y, int ldy, int n_img, int h, int w_,
                          int cin, int cout, int kh, int kw, int dil, int mode, int accumulate, void* stream);
long runet_conv_wgrad_fp16_workspace_floats(int n_img, int h, int w_, int cin, int cout, int kh, int kw, int dil, int transposed);
int runet_conv_wgrad_fp16(const float* x, int ldx, const float* dy, int ldy, float* dw, float* workspace, long workspace_floats,
                          int n_img, int h, int w_, int cin, int cout, int kh, int kw, int dil, int transposed, void* stream);

/* ---- harness helpers (Main_Final.py:577-578,596-597,648-649: `F.interpolate(outputs, size=masks.shape[-2:], mode='bilinear',
 *      align_corners=False)` when the model output and the mask differ in size; :82-117 standalone attention modules) ----
 * runet_bilinear_fwd: y[planes, ho, wo] = bilinear resize of x[planes, h, w] with ATen's align_corners=False source index
 *   (src = max(0, (dst + 0.5) * in/out - 0.5)).  runet_bilinear_bwd: dx[planes, h, w] = its adjoint applied to dy[planes, ho, wo]
 *   (gather form: fixed summation order, no atomics).
 * runet_mul_pixel: y[p, 0:c] = x[p, 0:c] * s[p]  (NHWC, one factor per pixel: SpatialAttention's output product). */
int runet_bilinear_fwd(const float* x, float* y, long planes, int h, int w, int ho, int wo, void* stream);
int runet_bilinear_bwd(const float* dy, float* dx, long planes, int h, int w, int ho, int wo, void* stream);
int runet_mul_pixel(const float* x, int ldx, const float* s, float* y, int ldy, long pixels, int c, void* stream);

/* ---- plain 2-class U-Net of the reference's older trainer (train_water_segmentation.py:209-288 `UNet`, :304 nn.CrossEntropyLoss;
 *      consumer predict_coastline.py:351): built from the kernels above plus
 * runet_nhwc_to_nchw: y[n][c][p] = x[(n*hw + p)*ld + c]  (the [N, classes, H, W] logits the module returns);
 * runet_ce_fwd / runet_ce_bwd: mean cross-entropy over all pixels of NCHW logits (2..8 classes) against int64 targets [N, H, W],
 *   ATen's log_softmax arithmetic; partials1024: 1024 doubles of scratch; gout: the scalar upstream gradient (device). */
int runet_nhwc_to_nchw(const float* x, int ld, float* y, int n_img, int c, long hw, void* stream);
int runet_ce_fwd(const float* logits_nchw, const long long* target, int n_img, int classes, long hw, double* partials1024, float* loss, void* stream);
int runet_ce_bwd(const float* logits_nchw, const long long* target, const float* gout, float* dlogits_nchw, int n_img, int classes, long hw,
                 void* stream);

/* ---- SegNet baseline of the reference's second comparison script (comne.py:84-211): 3x3 conv + BatchNorm2d + ReLU stacks joined by
 *      nn.MaxPool2d(2, 2, return_indices=True) and nn.MaxUnpool2d(2, 2) (comne.py:174-175, 177-211); Conv2d(64, 1, 3) + sigmoid head =
 *      runet_head3x3_fwd / _bwd above.  Pool index = the runet_maxpool2_fwd byte k = dy*2 + dx in the window (first maximum, NaN wins).
 * Unpool FORWARD (comne.py:197,200,203,206 self.unpool(x, idx, output_size)) is runet_maxpool2_bwd(accumulate=0): zeros, the value at
 *   its index - exactly nn.MaxUnpool2d's scatter (h, w = the unpooled size).
 * runet_bn_relu_maxpool2_fwd: y, idx = maxpool2(relu(t * scale + shift)) - an encoder block's last BatchNorm + ReLU and the pool that is its
 *   only consumer (comne.py:96-97 + 181, and :105-106 + 185, :117-118 + 189, :129-130 + 193); t is read once, the full-resolution
 *   activation is never written.  Same values and bytes as runet_bn_apply(relu=1) followed by runet_maxpool2_fwd.  h, w: t's size.
 * runet_bn_bwd_reduce_pooled / runet_bn_bwd_apply_pooled: runet_bn_bwd_reduce / runet_bn_bwd_apply (ReLU mask from x: relu_scale / relu_shift
 *   are the forward's scale / shift) whose incoming gradient is the POOLED gradient dpool [n, h/2, w/2, c] with the pool's bytes idx:
 *   g(n, y, x, c) = idx[n, y/2, x/2, c] == (y&1)*2 + (x&1) ? dpool[n, y/2, x/2, c] : 0 (autograd of :181 etc. into :96-97 etc.).
 *   Same bits as runet_maxpool2_bwd(accumulate=0) followed by the two plain calls.  h, w: x's size; workspace as runet_bn_bwd_reduce.
 * runet_maxunpool2_bwd: autograd of nn.MaxUnpool2d (comne.py:197,200,203,206), the gather dpool[n, ho, wo, c] = dU[n, 2ho + k/2, 2wo + k%2, c].
 *   h, w: dU's (unpooled) size.
 * All four: c a multiple of 4, h and w even, pixel strides multiples of 4. */
int runet_bn_relu_maxpool2_fwd(const float* t, int ldt, const float* scale, const float* shift, float* y, int ldy, unsigned char* idx,
                               int n_img, int h, int w, int c, void* stream);
int runet_bn_bwd_reduce_pooled(const float* dpool, int ldp, const unsigned char* idx, const float* x, int ldx, int n_img, int h, int w, int c,
                               const float* mean, const float* invstd, float* workspace, float* sums, const float* relu_scale,
                               const float* relu_shift, void* stream);
int runet_bn_bwd_apply_pooled(const float* dpool, int ldp, const unsigned char* idx, const float* x, int ldx, float* dx, int lddx, int n_img,
                              int h, int w, int c, const float* mean, const float* invstd, const float* scale, const float* sums, long m_total,
                              const float* relu_shift, void* stream);
int runet_maxunpool2_bwd(const float* du, int lddu, const unsigned char* idx, float* dpool, int ldp, int n_img, int h, int w, int c,
                         void* stream);

/* ---- YOLOSeg baseline (Main_Final.py:436-510): every BatchNorm2d is followed by nn.LeakyReLU(0.1, inplace=True); the backbone's four
 *      stages end in nn.MaxPool2d(2, stride=2) (:446, :452, :464, :476); seg_head is four ConvTranspose2d(k4, s2, p1) + BatchNorm2d +
 *      LeakyReLU (:481-498) and Conv2d(16, 1, 3) + sigmoid (runet_head3x3_fwd / _bwd above, :501, :506).
 * LeakyReLU(slope): act(z) = z > 0 ? z : z * slope with z = x * scale + shift (runet_bn_apply's fused multiply-add), the product in fp32 -
 *   the same bits as torch.nn.functional.leaky_relu(z, slope).  Not ReLU with slope 0 (that gives -0.0 for negative z).
 * runet_bn_apply_leaky: y = act(x * scale + shift) - runet_bn_apply(relu=0) followed by leaky_relu, in one pass.
 * runet_bn_bwd_reduce_leaky / runet_bn_bwd_apply_leaky: runet_bn_bwd_reduce / _apply of g = dy * (z > 0 ? 1 : slope), z recomputed from x
 *   with the forward's scale / shift (bitwise the forward's decision): the same bits as aten's leaky_relu backward on z followed by the plain
 *   calls (no act, no relu_scale / relu_shift).  Workspace, sums and m_total as there.
 * runet_bn_leaky_maxpool2_fwd: y, idx = maxpool2(act(t * scale + shift)) - a backbone stage's last BatchNorm + LeakyReLU and the pool
 *   that is its only consumer (:444-446, :450-452, :462-464, :474-476); t is read once, the full-resolution activation is never written.
 *   Same values and bytes as runet_bn_apply_leaky followed by runet_maxpool2_fwd (byte k = dy*2 + dx, first maximum, NaN wins).
 * runet_bn_bwd_reduce_pooled_leaky / runet_bn_bwd_apply_pooled_leaky: the LeakyReLU forms of runet_bn_bwd_reduce_pooled / _apply_pooled
 *   (pooled gradient + the pool's bytes, factor from x): the same bits as runet_maxpool2_bwd(accumulate=0) + the two calls above.
 * Pooled forms: c a multiple of 4, h and w (t's / x's size) even, pixel strides multiples of 4, tensors 16-byte and idx 4-byte aligned.
 * runet_convt4_igemm_stats: runet_convt4_igemm(RUNET_CONVT_FWD, accumulate 0) that also leaves the BatchNorm statistics partials of y
 *   for runet_bn_stats_finalize, stats [runet_convt4_igemm_stats_parts(n_img, h, w_, cout)][cout][3] = (count, mean, M2) per tile and
 *   output parity class; y has the same bits as the plain call.  h, w_: x's size. */
int runet_bn_apply_leaky(const float* x, int ldx, float* y, int ldy, long pixels, int hw, int c, const float* scale, const float* shift,
                         float slope, void* stream);
int runet_bn_bwd_reduce_leaky(const float* dy, int lddy, const float* x, int ldx, int n_img, int hw, int c, const float* mean, const float* invstd,
                              float* workspace, float* sums, const float* scale, const float* shift, float slope, void* stream);
int runet_bn_bwd_apply_leaky(const float* dy, int lddy, const float* x, int ldx, float* dx, int lddx, long pixels, int hw, int c, const float* mean,
                             const float* invstd, const float* scale, const float* sums, long m_total, const float* shift, float slope, void* stream);
int runet_bn_leaky_maxpool2_fwd(const float* t, int ldt, const float* scale, const float* shift, float slope, float* y, int ldy, unsigned char* idx,
                                int n_img, int h, int w, int c, void* stream);
int runet_bn_bwd_reduce_pooled_leaky(const float* dpool, int ldp, const unsigned char* idx, const float* x, int ldx, int n_img, int h, int w, int c,
                                     const float* mean, const float* invstd, float* workspace, float* sums, const float* scale, const float* shift,
                                     float slope, void* stream);
int runet_bn_bwd_apply_pooled_leaky(const float* dpool, int ldp, const unsigned char* idx, const float* x, int ldx, float* dx, int lddx, int n_img,
                                    int h, int w, int c, const float* mean, const float* invstd, const float* scale, const float* sums, long m_total,
                                    const float* shift, float slope, void* stream);
int runet_convt4_igemm_stats_parts(int n_img, int h, int w_, int cout);
int runet_convt4_igemm_stats(const float* x, int ldx, const float* w, const float* bias, float* y, int ldy, int n_img, int h, int w_, int cin,
                             int cout, float* stats, void* stream);

/* ---- SegFormer-Lite baseline (Extended_Baseline_Comparison.py:622-744).  Everything else it runs is shared: the 1x1 convolutions (q, kv,
 *      proj, fc1, fc2, linear_c*, linear_fuse) and the head's 3x3 through runet_conv_igemm & co., the patch embeddings' 7x7 s4 and 3x3 s2
 *      convolutions and the r x r s r key / value reductions through runet_conv2d_general / runet_conv_wgrad_general, BatchNorm + ReLU of the
 *      decoder, runet_outc_* (head's 1x1 + sigmoid), runet_bilinear_* (the probability map's resize).
 * runet_kv_attention_fwd / _bwd: EfficientSelfAttention's core (:647-662).  q [n, nq, c] (pixel stride ldq), kv [n, nk, 2c] (k = channels
 *   [0, c), v = [c, 2c)), heads split the channels contiguously (channel = head * 32 + j): c must be 32 * heads (head dimension 32, anything
 *   else is an error).  o [n, nq, c] = softmax((q k^T) * 32^-0.5) v per head, lse [n, heads, nq] the log-sum-exp of each query's scaled
 *   scores.  Any nq, any nk >= 1.  The backward takes the forward's o and lse, dO [n, nq, c] and an optional gradient of lse (dlse
 *   [n, heads, nq], may be NULL); it writes dq [n, nq, c] and dkv [n, nk, 2c]
 *   (no accumulation), bitwise reproducible (fixed summation order, no atomics).  workspace >= runet_kv_attention_bwd_workspace_floats
 *   floats (-1: bad shape).  fp32 throughout; pixel strides multiples of 4 floats, tensors 16-byte aligned.
 * runet_dwconv3x3_gelu_fwd: MixFFN's depthwise 3x3 (padding 1, groups = c, bias) + nn.GELU() (:628-633).  x [n, h, w, c], w [3][3][c] (the
 *   HWIO memory of the [c, 1, 3, 3] weight), b [c]; z = b + dwconv(x) (may be NULL: not kept), a = GELU(z), erf form.
 * runet_dwconv3x3_gelu_bwd_wgrad: g = da * GELU'(z) (g may be da itself, with the same stride) and dwdb [10c] = (dw [3][3][c] | db [c]),
 *   summed in a fixed order through `workspace` (>= runet_dwconv3x3_gelu_bwd_workspace_floats floats, -1: bad shape).  z NULL: z is
 *   recomputed from x, w and b (the nine neighbours of x are read for dw anyway), so the forward need not keep it.
 * runet_dwconv3x3_bwd_data: dx [n, h, w, c] = the depthwise convolution's data gradient of g.
 *   Depthwise: c a multiple of 4 up to 1024, pixel strides multiples of 4, tensors 16-byte aligned.
 * runet_bn_apply_gelu / runet_bn_bwd_reduce_gelu / runet_bn_bwd_apply_gelu: the patch embeddings' BatchNorm2d + nn.GELU() (:677-688), the GELU
 *   forms of runet_bn_apply_leaky / runet_bn_bwd_reduce_leaky / runet_bn_bwd_apply_leaky (the same kernels with another activation, the
 *   backward recomputes z = x * scale + shift with the forward's scale / shift).  Workspace, sums and m_total as there.
 * runet_bilinear_nhwc_fwd / _bwd: F.interpolate(mode='bilinear', align_corners=False) of NHWC maps (:737-739), x [n, h, w, 0:c] (pixel stride
 *   ldx) -> y [n, ho, wo, 0:c] (ldy): either side may be a channel slice of a wider buffer (the decoder resizes straight into its 1024-channel
 *   concat buffer).  The backward is the adjoint in gather form, fixed summation order, dx overwritten.  Same source-index rule as
 *   runet_bilinear_fwd / _bwd.  c a multiple of 4, pixel strides multiples of 4, pointers 16-byte aligned. */
long runet_kv_attention_bwd_workspace_floats(int n_img, int nq, int nk, int c, int heads);
int runet_kv_attention_fwd(const float* q, int ldq, const float* kv, int ldkv, float* o, int ldo, float* lse, int n_img, int nq, int nk, int c,
                           int heads, void* stream);
int runet_kv_attention_bwd(const float* q, int ldq, const float* kv, int ldkv, const float* o, int ldo, const float* dout, int lddo,
                           const float* lse, const float* dlse, float* dq, int lddq, float* dkv, int lddkv, float* workspace, long workspace_floats,
                           int n_img, int nq,
                           int nk, int c, int heads, void* stream);
int runet_dwconv3x3_gelu_fwd(const float* x, int ldx, const float* w, const float* b, float* z, int ldz, float* a, int lda, int n_img, int h,
                             int w_, int c, void* stream);
long runet_dwconv3x3_gelu_bwd_workspace_floats(int n_img, int h, int w_, int c);
int runet_dwconv3x3_gelu_bwd_wgrad(const float* x, int ldx, const float* w, const float* b, const float* da, int ldda, const float* z, int ldz,
                                   float* g, int ldg, float* workspace, long workspace_floats, float* dwdb, int n_img, int h, int w_, int c,
                                   void* stream);
int runet_dwconv3x3_bwd_data(const float* g, int ldg, const float* w, float* dx, int lddx, int n_img, int h, int w_, int c, void* stream);
int runet_bn_apply_gelu(const float* x, int ldx, float* y, int ldy, long pixels, int hw, int c, const float* scale, const float* shift,
                        void* stream);
int runet_bn_bwd_reduce_gelu(const float* dy, int lddy, const float* x, int ldx, int n_img, int hw, int c, const float* mean, const float* invstd,
                             float* workspace, float* sums, const float* scale, const float* shift, void* stream);
int runet_bn_bwd_apply_gelu(const float* dy, int lddy, const float* x, int ldx, float* dx, int lddx, long pixels, int hw, int c, const float* mean,
                            const float* invstd, const float* scale, const float* sums, long m_total, const float* shift, void* stream);
int runet_bilinear_nhwc_fwd(const float* x, int ldx, float* y, int ldy, int n_img, int h, int w, int ho, int wo, int c, void* stream);
int runet_bilinear_nhwc_bwd(const float* dy, int lddy, float* dx, int lddx, int n_img, int h, int w, int ho, int wo, int c, void* stream);

/* ---- HRNet-Water baseline (Extended_Baseline_Comparison.py:554-616; csrc/hrnet.hip).  Its convolutions (3x3, 3x3 stride 2 through
 *      runet_conv2d_general, 1x1), BatchNorm + ReLU and the unfused A/B partners (runet_bilinear_nhwc_*, runet_outc_*) are shared; these are
 *      the head and the two fusion branches with the 1x1 convolution / the BatchNorm affine moved across the bilinear interpolation (its
 *      weights sum to 1, so both commute with it).  fp32, NHWC, pixel strides multiples of 4 floats that cover the channels, tensors 16-byte
 *      aligned, c a multiple of 4 up to 1024.  No float atomics: every sum has a fixed order, results are bitwise reproducible.  The
 *      source-index rule is runet_bilinear_nhwc_fwd's (ATen align_corners=False) at out = 2 in and 4 in.
 * runet_hr_head_fwd: the head's BatchNorm + ReLU + Conv2d(c, 1, 1) at the 3x3 convolution's resolution (:599-601 with the 1x1 in front of the
 *   Upsample): z [n, h, w] = b[0] + sum_c w[c] * relu(t * scale[c] + shift[c]); t [n, h, w, c] (pixel stride ldt) is the convolution's raw output,
 *   the activated tensor is not written.
 * runet_up2_sigmoid_fwd: prob [n, 2h, 2w] (dense, the model's [N, 1, H, W] output) = sigmoid(bilinear x2 of z) (:600,:601).
 * runet_up2_sigmoid_bwd: dz [n, h, w] = the adjoint of that interpolation, in gather form, of dprob * prob * (1 - prob).
 * runet_hr_head_bwd_reduce: one pass over t and dz -> out [3c + 1] = (dgamma [c] | dbeta [c] | dw [c] | db): the BatchNorm sums
 *   (sum g * xhat | sum g) of g = dz * w[c] * (t * scale + shift > 0) in the (weight, bias) order of runet_bn_bwd_reduce,
 *   dw[c] = sum dz * relu(t * scale + shift), db = sum dz.  workspace >= runet_hr_head_bwd_workspace_floats floats (-1: bad shape).
 * runet_hr_head_bwd_apply: dt [n, h, w, c] (lddt) by runet_bn_bwd_apply's formula with g recomputed from dz, w and t (the activation's gradient
 *   is never materialised); sums = out[0 : 2c] of the reduce (all-reduced with m_total the global element count, or zeros in eval mode where
 *   dt = g * scale), m_total as there (0: the local pixel count).
 * runet_bn_bilinear_nhwc_fwd: a fusion branch's BatchNorm + Upsample (:589-590, :593-594) as y [n, s h, s w, 0:c] (ldy; may be a channel
 *   slice of the concat buffer, the neighbouring channels are not touched) = scale[c] * bilinear_s(x) + shift[c], x [n, h, w, c] the 1x1
 *   convolution's raw output, s = 2 or 4.
 * runet_bilinear_nhwc_bwd_sums: g [n, h, w, 0:c] (ldg) = the gather adjoint of the slice gradient dy [n, s h, s w, 0:c] (lddy) - the gradient of
 *   the BatchNorm's output - and in the same pass sums [2c] = (sum g * xhat | sum g) against x (mean, invstd: the saved statistics), what
 *   runet_bn_bwd_reduce(g, x) would compute; runet_bn_bwd_apply(g, x, act = NULL) then gives dx.  workspace >=
 *   runet_bilinear_nhwc_bwd_sums_workspace_floats floats (-1: bad shape). */
int runet_hr_head_fwd(const float* t, int ldt, const float* scale, const float* shift, const float* w, const float* b, float* z, int n_img, int h,
                      int w_, int c, void* stream);
int runet_up2_sigmoid_fwd(const float* z, float* prob, int n_img, int h, int w_, void* stream);
int runet_up2_sigmoid_bwd(const float* dprob, const float* prob, float* dz, int n_img, int h, int w_, void* stream);
long runet_hr_head_bwd_workspace_floats(int n_img, int h, int w_, int c);
int runet_hr_head_bwd_reduce(const float* dz, const float* t, int ldt, const float* scale, const float* shift, const float* w, const float* mean,
                             const float* invstd, float* workspace, long workspace_floats, float* out, int n_img, int h, int w_, int c,
                             void* stream);
int runet_hr_head_bwd_apply(const float* dz, const float* t, int ldt, const float* w, float* dt, int lddt, int n_img, int h, int w_, int c,
                            const float* mean, const float* invstd, const float* scale, const float* shift, const float* sums, long m_total,
                            void* stream);
int runet_bn_bilinear_nhwc_fwd(const float* x, int ldx, float* y, int ldy, const float* scale, const float* shift, int n_img, int h, int w_, int s,
                               int c, void* stream);
long runet_bilinear_nhwc_bwd_sums_workspace_floats(int n_img, int h, int w_, int c);
int runet_bilinear_nhwc_bwd_sums(const float* dy, int lddy, const float* x, int ldx, const float* mean, const float* invstd, float* g, int ldg,
                                 float* workspace, long workspace_floats, float* sums, int n_img, int h, int w_, int s, int c, void* stream);

/* ---- WaterNet baseline (Extended_Baseline_Comparison.py:378-473; csrc/water_index.hip).  Its encoder / decoder (3x3 convolutions, BatchNorm +
 *      ReLU, max-pool, the k2-s2 transposed convolutions, the CBAM channel attention, runet_outc_*) are shared; these are its front end,
 *      WaterIndexModule + torch.cat (:378-393, :458): Conv2d(3, 16, 1) -> BatchNorm2d(16) -> ReLU -> Conv2d(16, 4, 1) -> Sigmoid, cat([x, idx]).
 *      Every 16-channel tensor of that chain is recomputed per pixel in registers: z = W1 x + b1, y = z * scale + shift, a = relu(y),
 *      u = W2 a + b2, s = sigmoid(u).  fp32.  x is the NCHW image [n, 3, h, w] read through its four strides sn, sc, sh, sw (in floats, as
 *      runet_to_nhwc_pad).  Weights and their gradients in the physical (HWIO) layouts w1 [3][16], w2 [16][4].  No float atomics: every sum has
 *      a fixed order and the block count depends on the shape only, results are bitwise reproducible.
 * runet_water_index_parts: rows of the partials / workspace for a shape (-1: bad shape).  runet_water_index_workspace_floats: floats the two
 *   backward entries need (-1: bad shape).
 * runet_water_index_stats: part [runet_water_index_parts][16][3] = (count, mean, M2) of z over disjoint pixel sets (two passes per block over
 *   pixels held in registers), the layout runet_bn_stats_finalize consumes.
 * runet_water_index_fwd: out [n, h, w, 0:8] (pixel stride ldo, 16-byte aligned) = [R, G, B, s0, s1, s2, s3, 0], two 16-byte stores per pixel;
 *   scale / shift from runet_bn_stats_finalize (training) or runet_bn_finalize on the running buffers (eval).
 * runet_water_index_bwd_reduce: g = the gradient of channels 3..6 of that buffer (pointer to channel 3 of its first pixel, pixel stride ldg;
 *   any 4-byte alignment, e.g. a slice of enc1's data gradient).  du = g s (1 - s), da = W2^T du masked by y > 0.
 *   out [100] = (dgamma [16] = sum da * xhat | dbeta [16] = sum da | dW2 [16][4] = sum a du | db2 [4] = sum du).
 * runet_water_index_bwd_apply: dz = runet_bn_bwd_apply's formula on da (sums = out[0 : 32] of the reduce, or zeros in eval mode where
 *   dz = scale * da; m_total as there, 0: the local pixel count); out [64] = (dW1 [3][16] = sum x dz | db1 [16] = sum dz). */
int runet_water_index_parts(int n_img, int h, int w_);
long runet_water_index_workspace_floats(int n_img, int h, int w_);
int runet_water_index_stats(const float* x, long sn, long sc, long sh, long sw, int n_img, int h, int w_, const float* w1, const float* b1,
                            float* part, long part_floats, void* stream);
int runet_water_index_fwd(const float* x, long sn, long sc, long sh, long sw, int n_img, int h, int w_, const float* w1, const float* b1,
                          const float* scale, const float* shift, const float* w2, const float* b2, float* out, int ldo, void* stream);
int runet_water_index_bwd_reduce(const float* x, long sn, long sc, long sh, long sw, int n_img, int h, int w_, const float* g, int ldg,
                                 const float* w1, const float* b1, const float* scale, const float* shift, const float* w2, const float* b2,
                                 const float* mean, const float* invstd, float* workspace, long workspace_floats, float* out, void* stream);
int runet_water_index_bwd_apply(const float* x, long sn, long sc, long sh, long sw, int n_img, int h, int w_, const float* g, int ldg,
                                const float* w1, const float* b1, const float* scale, const float* shift, const float* w2, const float* b2,
                                const float* mean, const float* invstd, const float* sums, long m_total, float* workspace,
                                long workspace_floats, float* out, void* stream);
/* The element-wise steps of that chain in the reference's order that no shared kernel offers (the unfused A/B partner,
 * RUNET_NO_FUSED_WATER_INDEX=1), over c channels of NHWC views that may start at any channel (4-byte accesses):
 * y = sigmoid(u); du = dy * y * (1 - y); y = x (a channel-slice copy, the torch.cat). */
int runet_sigmoid_nhwc_fwd(const float* u, int ldu, float* y, int ldy, long pixels, int c, void* stream);
int runet_sigmoid_nhwc_bwd(const float* dy, int lddy, const float* y, int ldy, float* du, int lddu, long pixels, int c, void* stream);
int runet_copy_nhwc(const float* x, int ldx, float* y, int ldy, long pixels, int c, void* stream);

/* ---- MSWNet baseline (Extended_Baseline_Comparison.py:479-548; csrc/multiscale.hip).  Its convolutions (1x1, 3x3, the 5x5 through
 *      runet_conv2d_general), BatchNorm + ReLU, the 2x2 pools, the k2-s2 transposed convolutions and runet_outc_* are shared; these are the
 *      MultiScaleBlock's 3x3 stride-1 max-pool and its first level, MultiScaleBlock(3, 64), fused over the image.  fp32.  No float atomics:
 *      every sum has a fixed order and the block count depends on the shape only, results are bitwise reproducible.
 * runet_maxpool3s1_fwd: MaxPool2d(3, stride 1, padding 1) (:490) over NHWC views (pixel strides ldx, ldy >= c; any channel count and 4-byte
 *   alignment, 16-byte accesses where c, the strides and the pointers allow).  Padding counts as -inf.  idx (dense [n, h, w, c], may be NULL):
 *   one byte per output element, k = dy * 3 + dx of the first maximum in row-major window order; a NaN wins over everything (ATen's CPU rule).
 * runet_maxpool3s1_bwd: a gather - dx[p] = sum, in row-major order of the windows, of the dy of those of the <= 9 windows covering p whose
 *   winner byte points at p; accumulate != 0: added onto what dx holds.
 * The stem: x is the NCHW image [n, 3, h, w] read through its four strides (in floats, as runet_to_nhwc_pad).  Weights in their physical
 *   (HWIO) layouts w1 [1][1][3][16], w3 [3][3][3][16], w5 [5][5][3][16], w4 [1][1][3][16] (branch4's 1x1 on the 3x3 max-pool of x), biases
 *   b1, b3, b5, b4 [16].  t [64] = (w1 x + b1 | w3 * x + b3 | w5 * x + b5 | w4 maxpool3(x) + b4) per pixel (zero padding for the
 *   convolutions), y = t * scale + shift, e = relu(y); scale, shift, mean, invstd [64]: the four BatchNorms' vectors in branch order.  t is
 *   recomputed by the same FMAs in all four kernels and never written.  e, de, dt: NHWC views of 64 channels, pixel strides multiples of 4
 *   floats, pointers 16-byte aligned.
 * runet_ms_stem_parts: rows of the partials / workspace for a shape (-1: bad shape); runet_ms_stem_workspace_floats: floats
 *   runet_ms_stem_bwd_reduce needs (-1: bad shape).
 * runet_ms_stem_stats: part [4][runet_ms_stem_parts][16][3] = (count, mean, M2) of t per 8 x 32 pixel tile (two passes per block), one
 *   array per branch in the layout runet_bn_stats_finalize consumes (c = 16).
 * runet_ms_stem_fwd: e = relu(t * scale + shift).
 * runet_ms_stem_bwd_reduce: g = de where y > 0; sums [128] = (dgamma [64] = sum g * xhat | dbeta [64] = sum g).
 * runet_ms_stem_bwd_apply: dt = runet_bn_bwd_apply's formula on g (sums of the reduce, or zeros in eval mode where dt = scale * g; m_total
 *   as there, 0: the local pixel count). */
int runet_maxpool3s1_fwd(const float* x, int ldx, float* y, int ldy, unsigned char* idx, int n_img, int h, int w, int c, void* stream);
int runet_maxpool3s1_bwd(const float* dy, int lddy, const unsigned char* idx, float* dx, int lddx, int n_img, int h, int w, int c,
                         int accumulate, void* stream);
int runet_ms_stem_parts(int n_img, int h, int w_);
long runet_ms_stem_workspace_floats(int n_img, int h, int w_);
int runet_ms_stem_stats(const float* x, long sn, long sc, long sh, long sw, int n_img, int h, int w_, const float* w1, const float* w3,
                        const float* w5, const float* w4, const float* b1, const float* b3, const float* b5, const float* b4, float* part,
                        long part_floats, void* stream);
int runet_ms_stem_fwd(const float* x, long sn, long sc, long sh, long sw, int n_img, int h, int w_, const float* w1, const float* w3,
                      const float* w5, const float* w4, const float* b1, const float* b3, const float* b5, const float* b4, const float* scale,
                      const float* shift, float* e, int lde, void* stream);
int runet_ms_stem_bwd_reduce(const float* x, long sn, long sc, long sh, long sw, int n_img, int h, int w_, const float* w1, const float* w3,
                             const float* w5, const float* w4, const float* b1, const float* b3, const float* b5, const float* b4,
                             const float* scale, const float* shift, const float* de, int ldde, const float* mean, const float* invstd,
                             float* workspace, long workspace_floats, float* sums, void* stream);
int runet_ms_stem_bwd_apply(const float* x, long sn, long sc, long sh, long sw, int n_img, int h, int w_, const float* w1, const float* w3,
                            const float* w5, const float* w4, const float* b1, const float* b3, const float* b5, const float* b4,
                            const float* scale, const float* shift, const float* de, int ldde, const float* mean, const float* invstd,
                            const float* sums, long m_total, float* dt, int lddt, void* stream);

/* ---- Fast-SCNN baseline (comne.py:305-476; csrc/fastscnn.hip, csrc/dwsep.hip).  Its stem (3x3 stride 2 through runet_conv2d_general), 1x1
 *      convolutions and their gradients, BatchNorm + ReLU, runet_outc_* and runet_bilinear_nhwc_bwd_sums are shared; these are the pieces
 *      nothing else expresses.  NHWC fp32, pixel strides multiples of 4 floats that cover the channels (sources and destinations may be channel
 *      slices of wider buffers), tensors 16-byte aligned.  No float atomics: every sum has a fixed order, two runs give identical bits.
 * Depthwise 3x3, padding 1, stride 1 | 2, no bias (DepthwiseSeparableConv.depthwise, :310-311).  h, w_: the INPUT size, the output is
 *   ceil(h / stride) x ceil(w_ / stride); w [3][3][c] (the HWIO memory of the [c, 1, 3, 3] parameter); c a multiple of 4, at most 1024.
 *   runet_dw3_fwd: y = dwconv(x), taps in (r, s) order, one FMA per tap.
 *   runet_dw3_wgrad: dw [3][3][c] from x and dy (chunk partials in `workspace`, runet_dw3_wgrad_workspace_floats floats - -1: bad shape -,
 *     added in index order).  runet_dw3_dgrad: dx (input size) = the adjoint taps of dy, a gather.
 * Depthwise -> pointwise (:316-318) without the depthwise tensor, cin and cout multiples of 16, at most 128; wd [3][3][cin], wp [cin][cout] (the
 *   HWIO memory of the 1x1 weight):
 *   runet_dwsep_fwd: t = (dwconv(x)) wp, the product on the exact f32-input MFMA, and part [runet_dwsep_parts(n_img, h, w_, stride)][cout][3]
 *     = (count, mean, M2) of t per block of 64 output pixels, the layout runet_bn_stats_finalize consumes.
 *   runet_dwsep_wgrad_pw: dwp [cin][cout] = d^T dt with d = dwconv(x) recomputed by the forward's arithmetic (bit-equal); workspace:
 *     runet_dwsep_wgrad_pw_workspace_floats floats (-1: bad shape).
 * Pyramid pooling (PyramidPoolingFastSCNN, :343-371), bins 1 / 2 / 3 / 6.  The branch-major buffers hold [n * 1 | n * 4 | n * 9 | n * 36] rows
 *   (50 n rows), each branch a dense [n, b, b] image:
 *   runet_pyramid_pool_fwd: the four nn.AdaptiveAvgPool2d (:354) of x [n, h, w_, c] in one launch, ATen's windows
 *     [floor(i h / b), ceil((i + 1) h / b)).  runet_pyramid_pool_bwd: dx = direct (may be NULL; the concat's own slice of x, :364,371) + the four
 *     levels' dpooled / window area, a gather.
 *   runet_pyramid_upsample_fwd: the four F.interpolate(..., size=(h, w_), bilinear, align_corners=False) (:368) of a [50 n][cq] into the
 *     channel slices [j cq, (j + 1) cq) of y [n, h, w_, 4 cq] (runet_bilinear_nhwc_fwd's source-index rule); _bwd: the gather adjoint.
 * runet_ffm_fwd (FeatureFusionModule.forward, :421-427): y [n, s h, s w_, c] = relu((t_low * scale_low + shift_low) + (bilinear_s(t_high) *
 *   scale_high + shift_high)), t_high [n, h, w_, c] the raw convolution output of the high branch (the BatchNorm affine commutes with the
 *   interpolation), s an integer factor in 1..32.  runet_relu_mask_nhwc: g = dy where y > 0, else 0 (the ReLU's backward in front of the two
 *   branches' BatchNorm backward: the high one gathers it first, runet_bilinear_nhwc_bwd_sums takes no mask).
 * runet_up_sigmoid_fwd / _bwd (FastSCNN.forward, :474-476): prob [n, s h, s w_] = sigmoid(bilinear_s(z)) of the one-channel logit plane
 *   z [n, h, w_] and its gather adjoint, s in 1..32 (runet_up2_sigmoid_* is the s = 2 form with 16-byte stores). */
int runet_dw3_fwd(const float* x, int ldx, const float* w, float* y, int ldy, int n_img, int h, int w_, int c, int stride, void* stream);
long runet_dw3_wgrad_workspace_floats(int n_img, int h, int w_, int c, int stride);
int runet_dw3_wgrad(const float* x, int ldx, const float* dy, int lddy, float* workspace, long workspace_floats, float* dw, int n_img, int h,
                    int w_, int c, int stride, void* stream);
int runet_dw3_dgrad(const float* dy, int lddy, const float* w, float* dx, int lddx, int n_img, int h, int w_, int c, int stride, void* stream);
int runet_dwsep_parts(int n_img, int h, int w_, int stride);
int runet_dwsep_fwd(const float* x, int ldx, const float* wd, const float* wp, float* t, int ldt, float* part, int n_img, int h, int w_, int cin,
                    int cout, int stride, void* stream);
long runet_dwsep_wgrad_pw_workspace_floats(int n_img, int h, int w_, int cin, int cout, int stride);
int runet_dwsep_wgrad_pw(const float* x, int ldx, const float* wd, const float* dt, int lddt, float* workspace, long workspace_floats, float* dwp,
                         int n_img, int h, int w_, int cin, int cout, int stride, void* stream);
int runet_pyramid_pool_fwd(const float* x, int ldx, float* pooled, int ldp, int n_img, int h, int w_, int c, void* stream);
int runet_pyramid_pool_bwd(const float* dpooled, int ldp, const float* direct, int ldd, float* dx, int lddx, int n_img, int h, int w_, int c,
                           void* stream);
int runet_pyramid_upsample_fwd(const float* a, int lda, float* y, int ldy, int n_img, int h, int w_, int cq, void* stream);
int runet_pyramid_upsample_bwd(const float* dy, int lddy, float* da, int lda, int n_img, int h, int w_, int cq, void* stream);
int runet_ffm_fwd(const float* t_low, int ldl, const float* t_high, int ldh, const float* scale_low, const float* shift_low,
                  const float* scale_high, const float* shift_high, float* y, int ldy, int n_img, int h, int w_, int s, int c, void* stream);
int runet_relu_mask_nhwc(const float* dy, int lddy, const float* y, int ldy, float* g, int ldg, long pixels, int c, void* stream);
int runet_up_sigmoid_fwd(const float* z, float* prob, int n_img, int h, int w_, int s, void* stream);
int runet_up_sigmoid_bwd(const float* dprob, const float* prob, float* dz, int n_img, int h, int w_, int s, void* stream);

/* ---- prediction: CoastlineExtractor (predict_coastline.py:336-618), everything between the uint8 upload and the two result masks
 *      (csrc/coastline.hip).  Masks are dense uint8 [h][w]; tile origins are device int32 [n_tiles][2] = (y0, x0), may be negative or overhang.
 * runet_scene_to_tiles: the to-tensor conversion and Normalize of the transform (:360-362, :387) of a uint8 HWC RGB scene (row_stride bytes per row) cut into T x T
 *   tiles, written as the stem's padded NHWC input tiles [n_tiles][T][T][4] fp32 (channel 3 = 0): ((float)u8 / 255.0f - mean[c]) / std[c],
 *   two true divisions, no contraction - the bits of the host transforms.  Pixels outside the scene are 0.0f.
 * runet_argmax_stitch: torch.argmax(output, dim=1) (:392) read from the head's NHWC output as it stands (z4 [n_tiles][T][T][4], n_classes
 *   <= 4 valid): the class index of each tile's core (tile minus halo on each side, clipped to the scene) goes into the scene mask.  First
 *   maximal index; NaN is greater than everything, the first NaN wins (torch's CPU order).
 * runet_scene_to_tiles_nchw: the same arguments and the same arithmetic (one kernel body, the layout is its template parameter), written
 *   planar as [n_tiles][3][T][T] fp32 - the NCHW input every probability model's forward takes; no fourth channel; tiles 4-byte aligned.
 * runet_threshold_stitch: the binarisation of the 1-channel sigmoid models, `pred > threshold` with threshold 0.5 (Main_Final.py:521,
 *   comne.py:622, Extended_Baseline_Comparison.py:758, :920).  prob is [n_tiles][T][T] fp32 (one channel: NCHW and NHWC coincide); for each
 *   tile's core mask[y][x] = prob > threshold ? 1 : 0, compared in fp32 as torch compares an fp32 tensor with a scalar rounded to fp32.  An
 *   ordered compare: NaN gives 0 and +Inf gives 1, a probability equal to the threshold gives 0 - UNLIKE runet_argmax_stitch, where NaN wins.
 *   soft: NULL, or a dense [h][w] fp32 scene map that receives the same cores' probabilities bit for bit, NaN included (the map the
 *   reference's error / MAE figures are drawn from, Extended_Baseline_Comparison.py:954).  Pixels no core covers are left alone in both.
 *   Checked on the host before any launch: null pointers, tile <= 0, halo < 0 or 2 * halo >= tile, h * w beyond int32.
 * runet_resize_nearest_u8: cv2.resize(..., INTER_NEAREST) (:395-396) by OpenCV's index rule in IEEE double:
 *   sx = min((int)floor(x * (1.0 / ((double)dw / sw))), sw - 1), likewise for y.  dst 16-byte aligned.
 * runet_dilate_diff_u8: cv2.getStructuringElement(MORPH_ELLIPSE, (k, k)), cv2.dilate and `dilated_mask - water_mask` (:595-602) in one pass
 *   over a binary mask (any non-zero byte is water; outputs are 0 / 1): coast = dilate(mask) - mask, optionally dilated itself (NULL: not
 *   written; must share coast's address modulo 16), counts2 = {water pixels, coastline pixels} (device int32 [2], cleared by the call; integer
 *   atomics).  Outside the scene counts as 0.  k odd, 1 <= k <= 31.
 * runet_ellipse_spans: HOST ONLY, no device work - the structuring element as column spans, row i = [j1[i], j2[i]) (k ints each), OpenCV's
 *   MORPH_ELLIPSE rule: r = c = k / 2, dy = i - r, dx = round_half_even(c * sqrt((r*r - dy*dy) / (double)(r*r))), [max(c - dx, 0), min(c + dx + 1, k)). */
int runet_ellipse_spans(int k, int* j1, int* j2);
int runet_scene_to_tiles(const unsigned char* scene, int h, int w, long row_stride, const int* origins, int n_tiles, int tile, float mean0,
                         float mean1, float mean2, float std0, float std1, float std2, float* tiles, void* stream);
int runet_argmax_stitch(const float* z4, int n_tiles, int tile, int n_classes, const int* origins, int halo, unsigned char* mask, int h, int w,
                        void* stream);
int runet_scene_to_tiles_nchw(const unsigned char* scene, int h, int w, long row_stride, const int* origins, int n_tiles, int tile, float mean0,
                              float mean1, float mean2, float std0, float std1, float std2, float* tiles, void* stream);
int runet_threshold_stitch(const float* prob, int n_tiles, int tile, const int* origins, int halo, float threshold, unsigned char* mask,
                           float* soft, int h, int w, void* stream);
int runet_resize_nearest_u8(const unsigned char* src, int sh, int sw, unsigned char* dst, int dh, int dw, void* stream);
int runet_dilate_diff_u8(const unsigned char* mask, int h, int w, int k, unsigned char* coast, unsigned char* dilated, int* counts2,
                         void* stream);

/* ---- prediction: the contours of the coastline mask (predict_coastline.py:605-608: cv2.findContours(coastline_mask, RETR_EXTERNAL,
 *      CHAIN_APPROX_SIMPLE) and the `len(contour) > 10` filter) on the device, as parallel border following (csrc/contours.hip).  It replaces
 *      the host loop predict.trace_external_contours and returns its arrays: the outer border of every top-level component, in raster order of
 *      their start pixels, from the same first vertex, in the same order, collinear runs reduced the same way.  mask: dense uint8 [h][w], any
 *      non-zero byte is set, any address alignment, h * w < 2^31; it is only read and never goes to the host.
 * Formulation.  Directions d = 0..7 are E, NE, N, NW, W, SW, S, SE (y grows downwards).  Foreground is 8-connected, background 4-connected,
 *   outside the image is background.  A STATE (p, d) is a set pixel p whose neighbour in direction d is set ("at p, having come from there");
 *   its SUCCESSOR scans e = d + 1, d + 2, ... (mod 8) to the first set neighbour q of p and is (q, (e + 4) % 8); p is LEFT in direction e.  On
 *   the valid states this map is a bijection, so the states fall into disjoint cycles, one per border (outer or hole).  States exist only on
 *   pixels with a clear 4-neighbour (every border pixel is one; a spare state whose successor leaves them is its own successor), an isolated
 *   pixel carries one state that is its own successor.  START: (p0, d1) opens a contour iff p0's west neighbour is clear and 4-connected to
 *   the outside of the zero-padded image (the component is top-level), d1 is the first set neighbour of p0 clockwise from west (W, NW, N, NE,
 *   E, SE, S, SW) and p0 is the smallest pixel index of its cycle.  VERTEX: the pixel of state (p, d) is kept iff e != (d + 4) % 8, i.e. it is
 *   left in another direction than the previous pixel was; an isolated pixel is a one-vertex contour.  min_points > 0 drops every contour with
 *   <= min_points kept vertices, order preserved (the reference's filter is min_points = 10).
 * Two calls, caller-owned memory, all validation on the host before any device work:
 *   runet_contours_count: flags the border pixels, counts and numbers their states (prefix sum) and labels the background (union-find with
 *     minimum-index roots, integer atomicMin only) into `workspace` (>= runet_contours_workspace_bytes(h, w) bytes, 16-byte aligned; -1: bad
 *     shape); *n_states (device int64 [1], 8-byte aligned) receives the state count.  n_states = 0: no contour, nothing more to call.
 *   runet_contours_trace: with that count read back by the caller and `workspace` unchanged: successors, cycle minima and ranks by pointer
 *     jumping (a fixed ceil(log2(n_states)) rounds each, double-buffered), start marks, vertex flags, prefix sums, the filter, the packed
 *     result.  state_workspace: >= runet_contours_state_workspace_bytes(n_states) bytes (-1: n_states < 1 or >= 2^31), 16-byte aligned.  The
 *     packed result stands at its start: int32 {n, total, offsets [n + 1], points [total][2] = (x, y)}; contour i is points[offsets[i] :
 *     offsets[i + 1]]; n <= n_states, total <= n_states.
 * Every device loop is bounded by the data size (fixed jumping rounds, union-find walks over strictly decreasing indices).  No float atomics;
 * nothing depends on arrival order: two runs give the same bytes.  No host synchronisation except the caller's own reads: n_states between
 * the two calls, then {n, total}, then the packed result - three device-to-host transfers per mask.
 * runet_contours_workspace_bytes / runet_contours_state_workspace_bytes: HOST ONLY. */
long runet_contours_workspace_bytes(int h, int w);
long runet_contours_state_workspace_bytes(long n_states);
int runet_contours_count(const unsigned char* mask, int h, int w, void* workspace, long workspace_bytes, long* n_states, void* stream);
int runet_contours_trace(int h, int w, void* workspace, long workspace_bytes, long n_states, int min_points, void* state_workspace,
                         long state_workspace_bytes, void* stream);

/* ---- prediction: the polygons of those contours (predict_coastline.py:605-616; :612-615 is cv2.approxPolyDP(contour, 0.002 * arcLength))
 *      on the device, by the project's EXACT Douglas-Peucker rule (csrc/simplify.hip).  It is a rule of its own, not the float64 rule of
 *      predict.approx_poly_dp (whose ties are decided by rounding noise) and not a cv2 equality claim: every decision below is integer
 *      arithmetic or ONE correctly rounded IEEE-754 double operation, ties go to the first index, so predict.approx_poly_dp_exact (host,
 *      Python ints) and the kernels return the same lists bit for bit.
 * Input.  A closed contour of n integer vertices p[0..n), coordinates in [0, 46340]; every cyclic edge is a run: dx == 0, dy == 0 or
 *   |dx| == |dy|.  A vertex outside the range and an edge between two in-range vertices that is not a run are BAD INPUTS: counted, never
 *   guessed at.
 *   1. Arc length.  A = sum of |dx| + |dy| over the axis edges, D = sum of |dx| over the diagonal edges (exact integers, any order).
 *      L = (double)A + (double)D * 0x1.6a09e667f3bcdp+0, eps = eps_factor * L, thr = eps * eps: four double operations, each rounded on its
 *      own, NO fused multiply-add.
 *   2. Far vertex.  far = the first index that maximises |p[i] - p[0]|^2 (below 2^32).  far == 0: the result is [p[0]] (this covers n == 1);
 *      n == 2 keeps both vertices.
 *   3. Chain.  Positions 0..n with q[n] = p[0]; positions 0, far and n are kept; plain Douglas-Peucker on every segment (a, b) of
 *      consecutive kept positions with b - a >= 2.
 *   4. Distance numerator of interior position i.  ab = q[b] - q[a], ap = q[i] - q[a], den = ab.ab, dot = ap.ab:
 *        den == 0: N = |ap|^2, and 1 stands in for den below;   dot <= 0: N = |ap|^2 den;   dot >= den: N = |q[i] - q[b]|^2 den;
 *        otherwise N = (ap x ab)^2.  N = den * (squared distance to the CLIPPED segment) < 2^64: unsigned 64-bit, signed 64-bit cross product.
 *   5. Split.  k = the first interior position that maximises N; the segment splits at k iff (double)N > thr * (double)den (uint64 -> double
 *      rounds to nearest-even, the product is one rounded operation, the comparison is strict).
 *   6. Output.  The kept positions below n, in order.  No contour is dropped after simplification.
 * packed: the tracer's device result, int32 {n, total, offsets [n + 1], points [total][2]}, 4-byte aligned; n and total are the caller's (it
 *   has read them to cut the result) and must be the two leading words, offsets must rise from 0 to total - anything else counts as bad input.
 * workspace: >= runet_contours_simplify_workspace_bytes(n, total) bytes (-1 unless 0 <= n <= total < 2^30), 16-byte aligned.  At its start
 *   stands the HEAD, int32 {n, kept vertices, bad inputs, largest round count of any contour}; at byte
 *   runet_contours_simplify_result_offset() the packed result in the input's format, {n, kept, offsets [n + 1], points [kept][2]}.  The
 *   caller reads the head as its one size word.  bad inputs != 0: kept reads 0 and NOTHING is written past the head.
 * Formulation.  One workgroup per contour; level-synchronous rounds inside the kernel with workgroup barriers only (no grid barrier, no
 *   cooperative launch, no waiting on other workgroups).  In a round every interior position of a still-open segment computes its N, the
 *   segment takes (max N, first index) by integer atomicMax / atomicMin, decides, and its positions narrow their bounds or close.  Every
 *   round splits or closes every open segment: at most n rounds, the contour's recursion depth.  Contours of at most lds_max_vertices
 *   vertices (negative: the default; capped at the 2048 that fit LDS) keep their state in LDS, longer ones in the workspace; the results are
 *   the same bytes.  One prefix sum over the keep flags of all vertices gives slots and offsets, an emit pass writes the result.
 * All validation on the host before any device work: sizes, a finite eps_factor >= 0, workspace size and alignment.  n == 0 launches
 * nothing and writes an empty head and result.  No float atomics, nothing depends on arrival order: two runs give the same bytes.
 * runet_contours_simplify_workspace_bytes / runet_contours_simplify_result_offset: HOST ONLY. */
long runet_contours_simplify_workspace_bytes(long n, long total);
long runet_contours_simplify_result_offset(void);
int runet_contours_simplify(const int* packed, long n, long total, double eps_factor, int lds_max_vertices, void* workspace,
                            long workspace_bytes, void* stream);

/* ---- ENet baseline (comne.py:482-608; csrc/enet.hip, the rectangular launchers in csrc/conv_igemm.hip).  Its 1x1 and 3x3 (dilation 1..16)
 *      convolutions, BatchNorm + ReLU, the 2x2 max-pool and the k3-s2 transposed convolutions' gradients and A/B forward (the data gradient of a stride-2 convolution,
 *      runet_conv2d_general) are shared; these are the pieces nothing else expresses.  NHWC fp32, pixel strides multiples of 4 floats that cover
 *      the channels (sources and destinations may be channel slices of wider buffers, channels outside the slice stay untouched), tensors
 *      16-byte aligned, c a multiple of 4, at most 1024.  No float atomics: every sum has a fixed order, block counts depend on the shape only,
 *      two runs give identical bits.
 * runet_conv2d_rect / runet_conv_wgrad_rect: runet_conv2d_general / runet_conv_wgrad_general (modes RUNET_CONV_FWD and RUNET_CONV_DGRAD, strides
 *   1..8, kh, kw <= 8) with padding (pad_h, pad_w) and dilation (dil_h, dil_w) per axis: the asymmetric bottleneck's Conv2d (5, 1) padding
 *   (2, 0) and (1, 5) padding (0, 2).  Equal pads and dilations give runet_conv2d_general's bits.  runet_conv_wgrad_rect_workspace_floats: the
 *   split-K slabs for `pixels` output pixels (-1: bad shape).
 * runet_convt3_fwd: ConvTranspose2d(k3, s2, p1, output_padding 1) forward (decoder.0 / decoder.3), x [n, h, w_, cin] -> y [n, 2h, 2w_, cout], by
 *   output parity class: four GEMMs over the input pixels with 1 / 2 / 2 / 4 live taps (the data-gradient form of runet_conv2d_general runs
 *   9 taps per output pixel).  wq [9][cin][cout]: the parameter's physical [3][3][cin][cout] slabs in class order, written by
 *   runet_convt3_pack (device-to-device copies on `stream`).  bias [cout] may be NULL.
 * Initial block (InitialBlock.forward): x is the NCHW image [n, 3, h, w_] read through its four strides (in floats, as runet_to_nhwc_pad), h and
 *   w_ even; w [3][3][3][13], the HWIO memory of the [13, 3, 3, 3] parameter (13 output columns: no shared convolution entry takes it).
 *   runet_enet_initial_fwd: t [n, h/2, w_/2, 16] = (Conv2d 3x3 stride 2 padding 1 (x), zero padding, taps in (r, s, channel) order | the 2x2
 *     max of the three image channels, a subset of the same patch; a NaN wins), and part [runet_enet_initial_parts(n, h, w_)][16][3] =
 *     (count, mean, M2) of t per block of 256 output pixels, the layout runet_bn_stats_finalize consumes (-1: bad shape).
 *   runet_enet_initial_wgrad: dw [3][3][3][13] = sum over output pixels of patch (x) dt[..., 0:13], dt a 16-channel view; per-chunk partial slabs
 *     in `workspace` (runet_enet_initial_wgrad_workspace_floats floats, -1: bad shape), added in chunk order.  The image takes no gradient.
 * Bottleneck tail (BottleneckBlock.forward): t3 the raw output of conv3's convolution, idn the block's input (plain) or the raw output of
 *   conv_down's convolution (downsample: scale_d / shift_d / mean_d / invstd_d given, NULL otherwise), mask_nc [n][c] the Dropout2d keep mask
 *   already divided by 1 - p (NULL: none).
 *   runet_enet_tail_fwd: out = relu(mask * (t3 * scale3 + shift3) + id), id = idn or idn * scale_d + shift_d.
 *   runet_enet_tail_bwd_reduce: with g = dout where out > 0, sums [2c] = (sum g mask xhat3 | sum g mask), the local (dgamma | dbeta) of conv3's
 *     BatchNorm; downsample: sums [4c], followed by (sum g xhat_d | sum g) of conv_down's.  workspace: runet_enet_tail_bwd_workspace_floats
 *     floats (-1: bad shape).
 *   runet_enet_tail_bwd_apply: dt3 = runet_bn_bwd_apply's formula on g mask (sums: those of the reduce, or zeros in eval mode where
 *     dt3 = scale3 * g mask; m_total as there, 0: the local pixel count); did = the same for conv_down's BatchNorm on g (downsample) or g itself.
 * Head (decoder.6 + sigmoid): ConvTranspose2d(c, 1, 2, stride 2), w [2][2][c] (the physical memory of the [c, 1, 2, 2] parameter), bias [1];
 *   prob, dprob dense [n][2h][2w].
 *   runet_enet_head_fwd: prob[n, 2i + a, 2j + b] = sigmoid(bias + sum_c x[n, i, j, c] * w[a][b][c]), channels in index order.
 *   runet_enet_head_bwd: dz = dprob * prob * (1 - prob); dx[n, i, j, c] = sum_ab dz * w[a][b][c]; dw_db [4c + 1] = (dw [2][2][c] | db).
 *     workspace: runet_enet_head_bwd_workspace_floats floats (-1: bad shape). */
int runet_conv2d_rect(const float* x, int ldx, const float* w, const float* bias, float* y, int ldy, int n_img, int hin, int win, int cin,
                      int cin_w, int cout, int kh, int kw, int stride, int pad_h, int pad_w, int dil_h, int dil_w, int mode, int accumulate,
                      void* stream);
long runet_conv_wgrad_rect_workspace_floats(int pixels, int cin_w, int cout, int kh, int kw);
int runet_conv_wgrad_rect(const float* x, int ldx, const float* dy, int ldy, float* dw, float* workspace, long workspace_floats, int n_img,
                          int hin, int win, int cin, int cin_w, int cout, int kh, int kw, int stride, int pad_h, int pad_w, int dil_h,
                          int dil_w, void* stream);
int runet_convt3_pack(const float* w, float* wq, int cin, int cout, void* stream);
int runet_convt3_fwd(const float* x, int ldx, const float* wq, const float* bias, float* y, int ldy, int n_img, int h, int w_, int cin, int cout,
                     void* stream);
int runet_enet_initial_parts(int n_img, int h, int w_);
int runet_enet_initial_fwd(const float* x, long sn, long sc, long sh, long sw, const float* w, float* t, int ldt, float* part, int n_img, int h,
                           int w_, void* stream);
long runet_enet_initial_wgrad_workspace_floats(int n_img, int h, int w_);
int runet_enet_initial_wgrad(const float* x, long sn, long sc, long sh, long sw, const float* dt, int lddt, float* workspace,
                             long workspace_floats, float* dw, int n_img, int h, int w_, void* stream);
int runet_enet_tail_fwd(const float* t3, int ldt, const float* idn, int ldi, const float* scale3, const float* shift3, const float* scale_d,
                        const float* shift_d, const float* mask_nc, float* out, int ldo, int n_img, int h, int w_, int c, void* stream);
long runet_enet_tail_bwd_workspace_floats(int n_img, int h, int w_, int c, int downsample);
int runet_enet_tail_bwd_reduce(const float* dout, int lddo, const float* out, int ldo, const float* t3, int ldt, const float* idn, int ldi,
                               const float* mean3, const float* invstd3, const float* mean_d, const float* invstd_d, const float* mask_nc,
                               float* workspace, long workspace_floats, float* sums, int n_img, int h, int w_, int c, void* stream);
int runet_enet_tail_bwd_apply(const float* dout, int lddo, const float* out, int ldo, const float* t3, int ldt, const float* idn, int ldi,
                              const float* mean3, const float* invstd3, const float* scale3, const float* mean_d, const float* invstd_d,
                              const float* scale_d, const float* mask_nc, const float* sums, long m_total, float* dt3, int lddt, float* did,
                              int lddi, int n_img, int h, int w_, int c, void* stream);
int runet_enet_head_fwd(const float* x, int ldx, const float* w, const float* bias, float* prob, int n_img, int h, int w_, int c, void* stream);
long runet_enet_head_bwd_workspace_floats(int n_img, int h, int w_, int c);
int runet_enet_head_bwd(const float* dprob, const float* prob, const float* x, int ldx, const float* w, float* dx, int lddx, float* workspace,
                        long workspace_floats, float* dw_db, int n_img, int h, int w_, int c, void* stream);

/* ---- PSPNet baseline (comne.py:214-299; csrc/pspnet.hip).  Its stride-2 convolutions (runet_conv2d_general), the pyramid's pooling, 1x1
 *      convolutions and BatchNorms (runet_pyramid_pool_*, Fast-SCNN's entries at c = 512), the 3x3 convolution, the one-channel resize +
 *      sigmoid (runet_up_sigmoid_*) and the unfused A/B partners (runet_pyramid_upsample_*, runet_bn_apply, runet_outc_*) are shared.  fp32,
 *      NHWC, pixel strides multiples of 4 floats that cover the channels, tensors 16-byte aligned.  No float atomics: every sum has a fixed
 *      order, results are bitwise reproducible.  Source-index rule: runet_pyramid_upsample_fwd's (ATen align_corners=False, scale = b / size).
 * Tap planes: the pyramid half of final_conv.0 (:240 torch.cat + :279 Conv2d(1024, 512, 3, padding=1)) computed on the 50 cells per image.
 *   z [50 n][9 cout] (row stride ldz >= 9 cout) holds, branch-major like runet_pyramid_pool_fwd's rows, Z_j[n][cy][cx][r][s][0:cout] =
 *   P_j[n][cy][cx][:] . W[r][s][512 + 128 j : 512 + 128 (j + 1)][:]: a cell's activations times the nine taps' weight rows of its branch.
 *   runet_psp_taps_fwd: t [n, h, w_, 0:cout] (ldt; may be a channel slice, the neighbouring channels are not touched) += sum_j sum_(r, s)
 *     bilinear_(h, w_)(Z_j[..][r][s][:]) at (y + r - 1, x + s - 1), zero where that lies outside the map (the concat's zero padding).  Rows
 *     first (into LDS), then columns.
 *   runet_psp_taps_bwd: dz [50 n][9 cout] (lddz) = the adjoint in gather form of dt [n, h, w_, 0:cout] (lddt): columns first (into the
 *     workspace, >= runet_psp_taps_bwd_workspace_floats = n h 36 cout floats; -1: bad shape), then rows; one owner per element.
 *   runet_psp_taps_dp: da [50 n][cq] (lda) = the cells' gradient dP_j = dZ_j . Wtap_j^T of all four branches, dz as runet_psp_taps_bwd wrote it,
 *     wp [4 cq][9 cout] (row stride ldw) the pyramid rows of the weight with the input channel outermost (row j cq + k = branch j, channel k).
 *     The 9 cout deep contraction is split by tap (partials in the workspace, >= runet_psp_taps_dp_workspace_floats = 9 * 50 n cq floats;
 *     -1: bad shape) and summed in tap order; cq a multiple of 4 up to 256.
 * Head: final_conv.1-4 (:280-283 BatchNorm2d, ReLU, Dropout2d, Conv2d(c, 1, 1)) on the 3x3 convolution's raw output t [n, h, w_, c] (ldt);
 *   mask_nc [n][c] = the Dropout2d keep-mask / (1 - p), NULL in eval mode; c a multiple of 4 up to 1024.
 *   runet_psp_head_fwd: z [n, h, w_] = b[0] + sum_c w[c] * mask_nc[n][c] * relu(t * scale[c] + shift[c]); the activated tensor is not written.
 *   runet_psp_head_bwd_reduce: one pass over t and dz [n, h, w_] -> out [3c + 1] = (dgamma [c] | dbeta [c] | dw [c] | db): the BatchNorm sums
 *     (sum g * xhat | sum g) of g = dz * w[c] * mask_nc[n][c] * (t * scale + shift > 0), dw[c] = sum dz * mask_nc * relu(t * scale + shift),
 *     db = sum dz.  workspace >= runet_psp_head_bwd_workspace_floats floats (-1: bad shape).
 *   runet_psp_head_bwd_apply: dt [n, h, w_, c] (lddt) by runet_bn_bwd_apply's formula with g recomputed; sums = out[0 : 2c] of the reduce (or
 *     zeros in eval mode, where dt = g * scale), m_total as there (0: the local pixel count). */
int runet_psp_taps_fwd(const float* z, int ldz, float* t, int ldt, int n_img, int h, int w_, int cout, void* stream);
long runet_psp_taps_bwd_workspace_floats(int n_img, int h, int w_, int cout);
int runet_psp_taps_bwd(const float* dt, int lddt, float* dz, int lddz, float* workspace, long workspace_floats, int n_img, int h, int w_, int cout,
                       void* stream);
long runet_psp_taps_dp_workspace_floats(int n_img, int cq);
int runet_psp_taps_dp(const float* dz, int lddz, const float* wp, int ldw, float* workspace, long workspace_floats, float* da, int lda, int n_img,
                      int cq, int cout, void* stream);
int runet_psp_head_fwd(const float* t, int ldt, const float* scale, const float* shift, const float* mask_nc, const float* w, const float* b, float* z,
                       int n_img, int h, int w_, int c, void* stream);
long runet_psp_head_bwd_workspace_floats(int n_img, int h, int w_, int c);
int runet_psp_head_bwd_reduce(const float* dz, const float* t, int ldt, const float* scale, const float* shift, const float* mask_nc, const float* w,
                              const float* mean, const float* invstd, float* workspace, long workspace_floats, float* out, int n_img, int h, int w_,
                              int c, void* stream);
int runet_psp_head_bwd_apply(const float* dz, const float* t, int ldt, const float* mask_nc, const float* w, float* dt, int lddt, int n_img, int h,
                             int w_, int c, const float* mean, const float* invstd, const float* scale, const float* shift, const float* sums,
                             long m_total, void* stream);

/* ---- scene ingestion: the multi-band raster in front of the predictor (tif_to_image.py:42-171, train_water_segmentation.py:103-174,
 *      predict_coastline.py:425-581; csrc/scene_bands.hip).  bands is a planar device raster [n_bands][h][w] as GDAL's ReadAsArray stack gives
 *      it, dtype one of RUNET_BAND_*, read through band_stride / row_stride / elem_stride IN ELEMENTS (a row or column window of a larger raster
 *      needs no copy; strides must be positive and cover the extent), aligned to its element size, h * w < 2^31.  sel0..2 name the planes.
 * runet_band_percentiles: np.percentile(band, [q_lo, q_hi]) (method "linear") of the first n_sel (1..3) selected planes -> pct, device float64
 *   [n_sel][2].  The HOST computes numpy's ranks and weights, vi = (n - 1) * (q / 100), k = floor(vi), g = vi - k, and passes k_lo, g_lo, k_hi,
 *   g_hi; the device finds the exact order statistics of ranks k and min(k + 1, n - 1) (radix select on an order-preserving key, integer
 *   atomics only: bits do not depend on arrival order) and interpolates by numpy's _lerp in float64 without contraction: a + (b - a) * g,
 *   replaced by b - (b - a) * (1 - g) where g >= 0.5.  b - a is taken as numpy takes it, in the band's own dtype (int16 wraps, float32
 *   rounds); wide_diff != 0 takes it in float64 instead, which is np.percentile of band.astype(float64) (normalize_image_for_display).
 *   -0.0 and +0.0 are one value (+0.0).  float32: nonfinite (device int32 [1], cleared by the call, 0 for the other dtypes) counts the NaNs
 *   and infinities of the selected planes; the percentiles of such a plane are unspecified.  workspace: device memory of at least
 *   runet_band_percentiles_workspace(n_sel) BYTES (host only, -1: bad n_sel), 8-byte aligned, cleared by the call.  No host synchronisation.
 * runet_band_stretch_u8: out, interleaved uint8 [h][w][3] with out_row_stride bytes per row (any address phase), from the three selected
 *   planes and pct [3][2]; per pixel, in float64, true division, no contraction:
 *     s = min(max((double(v) - p_lo) / (p_hi - p_lo) * 255, 0), 255)
 *   mode 0 "water" (enhance_image_for_water, enhance_image(enhance_water=True)): channel 0 only, s < 100 -> s * 0.7;  mode 1 "rgb"
 *   (enhance_image(enhance_water=False)): nothing more;  mode 2 "display" (normalize_image_for_display): a channel whose p_hi - p_lo > 0 does
 *   not hold takes s = min(max(double(v), 0), 255).  The cast follows the reference's detour through the input dtype: integer inputs truncate
 *   s toward zero, float32 input rounds s to float32 first and truncates that.  A constant band in modes 0 / 1 divides by zero, which the
 *   reference leaves to an undefined float -> integer cast; here a NaN quotient (0 / 0, or a NaN input) writes 0, +inf writes 255 and -inf 0.
 * Both validate on the host and return non-zero before any device work.
 * runet_band_percentiles_timed: MEASUREMENT ONLY (tools/bench_scene.py) - the same call with a device event around every selection pass (one
 *   counting launch + one scan launch); it synchronises the host and writes the passes' milliseconds to the HOST array pass_ms [4]. */
#define RUNET_BAND_U8 0
#define RUNET_BAND_U16 1
#define RUNET_BAND_I16 2
#define RUNET_BAND_F32 3
long runet_band_percentiles_workspace(int n_sel);
int runet_band_percentiles(const void* bands, int dtype, int n_bands, int h, int w, long band_stride, long row_stride, long elem_stride, int sel0,
                           int sel1, int sel2, int n_sel, long k_lo, double g_lo, long k_hi, double g_hi, int wide_diff, double* pct,
                           int* nonfinite, void* workspace, long workspace_bytes, void* stream);
int runet_band_percentiles_timed(const void* bands, int dtype, int n_bands, int h, int w, long band_stride, long row_stride, long elem_stride,
                                 int sel0, int sel1, int sel2, int n_sel, long k_lo, double g_lo, long k_hi, double g_hi, int wide_diff,
                                 double* pct, int* nonfinite, void* workspace, long workspace_bytes, void* stream, float* pass_ms);
int runet_band_stretch_u8(const void* bands, int dtype, int n_bands, int h, int w, long band_stride, long row_stride, long elem_stride, int sel0,
                          int sel1, int sel2, const double* pct, int mode, unsigned char* out, long out_row_stride, void* stream);

/* ---- device-resident dataset (csrc/input_pipeline.hip, device_data.py).  The reference's dataset decodes, rasterises and LANCZOS-resizes
 *      every sample on every epoch (Main_Final.py:40-54), and its training script augments on the host with torchvision
 *      (train_water_segmentation.py:313-321: RandomHorizontalFlip, RandomRotation(10), ColorJitter(0.1, 0.1, 0.1), the / 255 conversion to float, Normalize).  Here
 *      a sample is built once into a uint8 cache on the device and every batch is assembled there.  All of it is exact against PIL, byte for
 *      byte; every table comes from the host (device_data.resample_tables / nearest_table / rotation_words, PIL's rules in double precision),
 *      the kernels apply them and clamp what they read from a table to the source.  All validation happens on the host before any device
 *      work and reports through runet_last_error.
 * runet_resample8_rows / runet_resample8_cols: the horizontal and the vertical pass of Image.resize on dense HWC uint8, c = 1 or 3, source and
 *   destination at any byte address.  bounds int32 [out][2] = (first source index, tap count), coeffs int32 [out][ksize] = 22-bit fixed-point
 *   weights (1 <= ksize <= 255), both 4-byte aligned.  Per output byte: clamp((2^21 + sum_t coeffs[o][t] * src[first + t]) >> 22, 0, 255),
 *   int32 accumulator, arithmetic shift.  The filter (LANCZOS, BILINEAR) is in the tables alone.  rows: [h][w_in][c] -> [h][w_out][c];
 *   cols: [h_in][w][c] -> [h_out][w][c], h_out <= 65535.  An image stays below 2^31 bytes.
 * runet_gather2d_u8: dst[y][x] = src[ytab[y]][xtab[x]] on one dense uint8 plane (Image.resize(NEAREST) of the mask); dst 4-byte aligned.
 * runet_batch_gray_sums: sums[i] (device int64 [b], 8-byte aligned, cleared by the call) = the integer sum of L = (19595 R + 38470 G + 7471 B
 *   + 32768) >> 16 over sample i as it stands in front of its contrast step: gathered through flip and rotation, the jitter steps that come
 *   before contrast in its order applied.  Integer adds only (64-bit atomics): two runs give the same bytes.
 * runet_batch_assemble: images uint8 [m][s][s][3] and masks uint8 [m][s][s] (the cache, 4-byte aligned), index int32 [b] (any order,
 *   repeats allowed; an index outside 0..m-1 is clamped), 1 <= s <= 4096, 1 <= b <= 65535 -> out_images float32 [b][3][s][s], out_masks float32
 *   [b][1][s][s] (16-byte aligned).  Without geom / factors / sums (all three NULL): out = ((byte / 255) - mean[c]) / std[c] in correctly
 *   rounded float32 operations, mask = (float)byte.  With them (all three given), per output pixel (x, y) of sample i:
 *     geom int32 [b][8] = {flip, a0, a1, a2, a3, a4, a5, order}: source ((a2 + y a1 + x a0) >> 16, (a5 + y a4 + x a3) >> 16) of the flipped
 *       image (Image.rotate's 16.16 affine_fixed after transpose(FLIP_LEFT_RIGHT)); outside the image: 0.
 *     order = step0 | step1 << 2 | step2 << 4 with 0 brightness, 1 contrast, 2 saturation; factors float32 [b][3] in that numbering.  Each
 *       step is Image.blend(degenerate d, image a, f): t = float32(d) + float32(f * float32(a - d)), no fused multiply-add; trunc(t) for
 *       0 <= f <= 1, else clamped to 0..255 first; the byte goes on to the next step.  d = 0 (brightness), the pixel's L (saturation),
 *       int(sums[i] / s^2 + 0.5) in double (contrast: ImageStat's mean of the whole current image, zero-filled corners included).
 *     mask_mode 1 ("follow"): the mask takes the same gather, fill 0;  0 ("fixed"): the mask is left alone, as the reference does. */
int runet_resample8_rows(const unsigned char* src, int h, int w_in, int c, const int* bounds, const int* coeffs, int ksize, unsigned char* dst,
                         int w_out, void* stream);
int runet_resample8_cols(const unsigned char* src, int h_in, int w, int c, const int* bounds, const int* coeffs, int ksize, unsigned char* dst,
                         int h_out, void* stream);
int runet_gather2d_u8(const unsigned char* src, int sh, int sw, const int* ytab, const int* xtab, unsigned char* dst, int dh, int dw,
                      void* stream);
int runet_batch_gray_sums(const unsigned char* images, int m, int s, const int* index, int b, const int* geom, const float* factors, long* sums,
                          void* stream);
int runet_batch_assemble(const unsigned char* images, const unsigned char* masks, int m, int s, const int* index, int b, float mean0,
                         float mean1, float mean2, float std0, float std1, float std2, const int* geom, const float* factors, const long* sums,
                         int mask_mode, float* out_images, float* out_masks, void* stream);

/* ---- report arrays: what the reference's two figures show, computed on the device (csrc/report.hip, report.py).  The analysis report of one
 *      extraction (predict_coastline.py:708-835) and the error maps of the model comparison (Extended_Baseline_Comparison.py:882-959) are
 *      numpy on the host there.  Every result below equals numpy's bit for bit (tests/report_ref.py restates the rules).  h * w < 2^31.  No
 *      floating-point atomics; integer atomics only, so the bits do not depend on arrival order.  All validation happens on the host before
 *      any device work; no call synchronises the host.
 * runet_report_overlay_u8 (:708-730, the "combined" panel): image and out dense interleaved uint8 [h][w][3], water and coast dense uint8
 *   [h][w], all 4-byte aligned; table uint8 [3][256] on the device.  Per pixel: coast == 1 -> (255, 255, 255); else water == 1 -> channel c
 *   becomes table[c][v]; else unchanged (mask bytes other than 1 leave the pixel alone; coast wins over water).  The HOST fills the table
 *   from the reference's own expression, the C cast to uint8 (truncation) of float64(v) * 0.6 + (0, 100, 200)[c] * 0.4.  5 bytes read and
 *   3 written per pixel.
 * runet_ndwi_stats / runet_ndwi_hist (:789-813, the NDWI histograms of the water and the non-water pixels): bands as in the scene ingestion
 *   (planar, strided, RUNET_BAND_*), n_bands >= 4, green = plane 1, NIR = plane 3 (GetRasterBand(2) and (4)); mask dense uint8 [h][w].
 *   Per pixel in float64, each operation rounded once, true division, no contraction:  x = (g - n) / ((g + n) + 1e-8).
 *   Class 0 "water" is mask == 1, class 1 "rest" is mask == 0; other mask bytes count nowhere.
 *   stats, device 8 x 64-bit words, written whole by the call: {count water, count rest, non-finite x over both classes, min key water, max
 *     key water, min key rest, max key rest, 0}.  A non-finite x is counted in word 2 only.  key(x) = the bits of x with -0.0 taken as +0.0,
 *     then ~bits for a negative x and bits | 2^63 otherwise: unsigned order = numeric order; an empty class keeps min key 2^64 - 1 and max
 *     key 0.  Integer atomics (add, min, max).
 *   hist: edges, device float64 [2][bins + 1] (class-major, rising: np.linspace(min, max, bins + 1) built by the host, as np.histogram
 *     builds them), 2 <= bins <= 256; counts, device 64-bit [2][bins], cleared by the call.  Bin i holds edges[i] <= x < edges[i + 1], the
 *     last bin also x == edges[bins]; computed numpy's way (the equal-bin path of np.histogram): i = trunc(((x - first) / (last - first)) *
 *     bins), i == bins -> bins - 1, then i - 1 if x < edges[i], then i + 1 if x >= edges[i + 1] and i != bins - 1.  x outside [first, last]
 *     or NaN counts nowhere.  Histograms private to a wave in LDS, merged with integer atomics.
 *   stats reads 2 elements + 1 byte per pixel and writes nothing but the eight words; hist the same plus 2 * bins counts.
 * runet_rgb_hist_u8 (:821-829, the fallback below four bands): image dense interleaved uint8 [h][w][3], 4-byte aligned -> hist, device
 *   64-bit [3][256], cleared by the call: the exact count of every byte value per channel.  3 bytes read per pixel.  The host folds it into
 *   np.histogram's bins (report.py: fold_byte_histogram).
 * runet_error_overlays (Extended_Baseline_Comparison.py:882-959): images fp32 [n][3][h][w] (normalised), prob and masks fp32 [n][1][h][w],
 *   1 <= n <= 65535.  One pass, per pixel and channel c, fp32 operations each rounded once, no contraction:
 *     vis  fp32 [n][h][w][3] = clamp(fl32(fl32(x * std[c]) + mean[c]), 0, 1) with v < 0 -> 0, v > 1 -> 1 (NaN stays NaN)          (:885)
 *     p = prob > threshold (ordered: NaN is not);  class TP: p and g == 1, FP: p and g == 0, FN: not p and g == 1, TN: not p and g == 0;
 *       a mask value that is neither 0 nor 1 (NaN included) puts the pixel in a fifth class "none"                                  (:920-927)
 *     overlay fp64 [n][h][w][3] = float64(fl32(fl32(0.4) * vis)) + colours[class][c], colours device float64 [5][3] = 0.6 * the class
 *       colour as the HOST computes it in float64 (TP .2 .8 .2, FP .9 .2 .2, FN .2 .2 .9, TN .9 .9 .9, none 0 0 0)                 (:929-935)
 *     err fp32 [n][h][w] = |prob - masks| in fp32                                                                                  (:954)
 *     counts, device 64-bit [n][5] (cleared by the call) = the pixels of each class (TP, FP, FN, TN, none); integer atomics         (:940-941)
 *     sums, device float64 [n] = S, the sum of err in float64 in this fixed order (the host's mae = S / (h * w); np.mean at :957 adds the
 *       fp32 values pairwise in fp32 and differs by that rounding only): pixels are cut into chunks of 1024, chunk b = [1024 b, 1024 (b + 1)),
 *       err beyond h * w counting as 0.  In a chunk, t = 0..255: d[t] = ((e[t] + e[t + 256]) + e[t + 512]) + e[t + 768]; the 256 d fall into
 *       four groups of 64 consecutive t, each folded by a[t] += a[t + o] for o = 32, 16, 8, 4, 2, 1 to a[0]; chunk sum = ((a0 + a1) + a2) +
 *       a3.  Then lane l = 0..63 adds the chunk sums l, l + 64, l + 128, ... in that order from 0.0, and the 64 lanes fold the same way.
 *   workspace: at least runet_error_overlays_workspace_bytes(n, h, w) BYTES (host only; -1: bad shape), 8-byte aligned: the chunk sums.
 *   20 bytes read and 40 written per pixel (12 vis + 24 overlay + 4 err). */
int runet_report_overlay_u8(const unsigned char* image, const unsigned char* water, const unsigned char* coast, int h, int w,
                            const unsigned char* table, unsigned char* out, void* stream);
int runet_ndwi_stats(const void* bands, int dtype, int n_bands, int h, int w, long band_stride, long row_stride, long elem_stride,
                     const unsigned char* mask, long* stats, void* stream);
int runet_ndwi_hist(const void* bands, int dtype, int n_bands, int h, int w, long band_stride, long row_stride, long elem_stride,
                    const unsigned char* mask, const double* edges, int bins, long* counts, void* stream);
int runet_rgb_hist_u8(const unsigned char* image, int h, int w, long* hist, void* stream);
long runet_error_overlays_workspace_bytes(int n, int h, int w);
int runet_error_overlays(const float* images, const float* prob, const float* masks, int n, int h, int w, float threshold, float mean0,
                         float mean1, float mean2, float std0, float std1, float std2, const double* colours, float* vis, double* overlay,
                         float* err, long* counts, double* sums, void* workspace, long workspace_bytes, void* stream);

/* ---- exact Euclidean distance transform and the statistics of a distance map (csrc/edt.hip, boundary.py): the primitive behind the
 *      coastline-accuracy scores (mean / RMS / worst deviation, share within t pixels, boundary F-score, Boundary IoU).  The reference has
 *      region scores only (Main_Final.py:527-547 per image, train_water_segmentation.py:355 for the empty union); nothing there measures a
 *      coastline.  The squared distance between two pixels is an integer, so every result below is defined exactly: no ties, no tolerance
 *      (tests/edt_ref.py restates the rules in numpy).  All arithmetic of the transform is integer, 64-bit where parabola intersections
 *      are formed; the one floating-point sum has a fixed order; integer atomics only.  All validation happens on the host before any
 *      device work; no call synchronises the host.  1 <= h, w <= 32768, so that (h - 1)^2 + (w - 1)^2 < RUNET_EDT_NONE.
 * runet_edt_workspace_bytes: host only; the BYTES either call below needs for n images of h x w (2 per pixel, at least 8 per 1024 pixels);
 *   -1: bad shape, or a batch whose grid would not fit.
 * runet_edt_sq_u8: mask uint8, image i's pixel (y, x) at mask[i * image_stride + y * row_stride + x] (row_stride >= w; image_stride >= an
 *   image's extent where n > 1), any byte address.  A feature pixel is a non-zero byte (invert == 0) or a zero byte (invert != 0).
 *   d2, dense int32 [n][h][w]:  d2[i][y][x] = min over the feature pixels (y', x') of image i of (x - x')^2 + (y - y')^2, so 0 on a feature
 *   pixel itself, and RUNET_EDT_NONE everywhere in an image without a feature pixel.  Only pixels inside the image are features: the frame
 *   around it is neither water nor land.
 *   Two launches.  Pass 1, a wave per row: g = |x - x'| to the nearest feature of the same row, -1 where the row has none (a state of its
 *   own: such a row never enters the arithmetic of pass 2).  Pass 2, a thread per column, 64 adjacent columns per wave: the lower envelope
 *   of the parabolas (y - y')^2 + g(y')^2 over the rows y' with g >= 0, first a stack of (row, g, first row owned) built top to bottom, then
 *   the column filled bottom to top.  It runs in place: a column of d2 holds g, then the stack, then the result; the workspace holds the
 *   first-row-owned values, uint16 [n][h][w].  Every loop is bounded by h or w.  Two runs give the same bytes.
 *   1 mask byte read per pixel; d2 written twice and read once in pass 1, read once and written once in pass 2 plus the stack traffic
 *   (at most 6 bytes written and 6 read per stack entry).
 * runet_edt_stats: one pass over d2 (dense int32 [n][h][w]).  select: dense uint8 [n][h][w], non-zero = the pixel takes part; NULL = every
 *   pixel does.  tol_sq: HOST array of n_tol squared tolerances (each >= 0), 0 <= n_tol <= 8, read during the call; may be NULL when
 *   n_tol == 0.  counts, device 64-bit [n][4 + n_tol], cleared by the call:
 *     [0] selected pixels;  [1] selected pixels with d2 == RUNET_EDT_NONE, which count in nothing below;  [2] max d2;  [3] sum of d2;
 *     [4 + t] pixels with d2 <= tol_sq[t].
 *   sums, device float64 [n] = S, the sum of e = sqrt((double)d2) (correctly rounded, np.sqrt) over the same pixels, in this fixed order:
 *     pixels are cut into chunks of 1024, chunk b = [1024 b, 1024 (b + 1)); e is 0.0 for a pixel that is not selected, is RUNET_EDT_NONE
 *     or lies beyond h * w.  In a chunk, t = 0..255: d[t] = ((e[t] + e[t + 256]) + e[t + 512]) + e[t + 768]; the 256 d fall into four
 *     groups of 64 consecutive t, each folded by a[t] += a[t + o] for o = 32, 16, 8, 4, 2, 1 to a[0]; chunk sum = ((a0 + a1) + a2) + a3.
 *     Then lane l = 0..63 adds the chunk sums l, l + 64, l + 128, ... in that order from 0.0, and the 64 lanes fold the same way.
 *   workspace: the chunk sums, 8-byte aligned.  4 bytes (+ 1 with select) read per pixel; nothing written but counts, sums and chunk sums. */
#define RUNET_EDT_NONE 2147483647
long runet_edt_workspace_bytes(int n, int h, int w);
int runet_edt_sq_u8(const unsigned char* mask, int n, int h, int w, long row_stride, long image_stride, int invert, int* d2, void* workspace,
                    long workspace_bytes, void* stream);
int runet_edt_stats(const int* d2, const unsigned char* select, int n, int h, int w, const int* tol_sq, int n_tol, long* counts, double* sums,
                    void* workspace, long workspace_bytes, void* stream);

/* ---- connected components of a byte mask, their areas, and the area filter in front of the coastline (csrc/ccl.hip, components.py).  The
 *      reference traces coastlines on `dilated - water` with cv2.findContours(RETR_EXTERNAL) and keeps every contour of more than 10 points
 *      (predict_coastline.py:583-618) from a mask thresholded at Main_Final.py:521: every speck of water inland and every hole of land at
 *      sea becomes a coastline.  These calls stand in front of that step.  Everything is an integer with an exact definition
 *      (tests/ccl_ref.py restates the rules with a flood fill): there is no tolerance.
 *      Determinism: every merge is an integer minimum (atomicMin on a parent), every count an integer sum, every box an integer minimum or
 *      maximum, so the result is independent of scheduling by construction: two runs give the same bytes.  32-bit integer atomics on vector
 *      memory only; no cooperative launch, no grid-wide barrier, no loop that waits on another workgroup: parents only decrease, so every
 *      loop descends and ends.  All validation (null pointers, connectivity, shapes, workspace size, alignment) happens on the host before
 *      any device work and returns non-zero with a runet_last_error() text; every call is asynchronous on `stream`; none synchronises the
 *      host.  1 <= h, w <= 32768, so h * w <= 2^30 and index + 1 fits int32.  Pixel (y, x) of an image has the linear index y * w + x;
 *      indices and labels are per image, and the images of a batch are independent.
 * Definitions.  A feature pixel is a non-zero byte (invert == 0) or a zero byte (invert != 0).  Two feature pixels of one image are
 *   neighbours when |dx| + |dy| == 1 (connectivity 4) or max(|dx|, |dy|) == 1 (connectivity 8); only pixels inside the image exist, so a
 *   row's last pixel and the next row's first are not neighbours.  A component is a class of the transitive closure of "neighbour".  Its
 *   root is its pixel of smallest linear index, its label is root index + 1.
 * runet_ccl_workspace_bytes: host only; the BYTES runet_ccl_label_u8 and runet_ccl_table need for n images of h x w (4 per pixel + 4 per
 *   1024 pixels, rounded up to 8); -1: bad shape, or a batch that one call cannot take (n * h * w > 2^40 or a grid that would not fit).
 * runet_ccl_label_u8: mask uint8, image i's pixel (y, x) at mask[i * image_stride + y * row_stride + x] (row_stride >= w; image_stride >= an
 *   image's extent where n > 1), any byte address: the stride contract of runet_edt_sq_u8, so a crop of a larger mask is read in place.
 *   connectivity: 4 or 8.  labels, dense int32 [n][h][w]: 0 on a non-feature pixel, otherwise the label of the pixel's component.
 *   Three launches: a block labels a 64 x 64 tile in LDS and writes every pixel's tile-local root as a global index; a thread per pixel of
 *   the tile border rows and columns unites it with its neighbours across the border (the diagonal pairs at tile corners included); every
 *   pixel walks to its root.  1 mask byte read per pixel; labels written once, read once and written again where the root changed.
 * runet_ccl_areas: labels as written above.  areas, dense int32 [n][h][w], and frame, dense uint8 [n][h][w], are written whole by the call:
 *   at a component's root pixel (linear index label - 1) areas holds the component's pixel count and frame its contact with the image's
 *   edge, bit 0 = a pixel with y == 0, bit 1 = y == h - 1, bit 2 = x == 0, bit 3 = x == w - 1; every other pixel holds 0 in both.
 * runet_ccl_filter_u8: a component is SELECTED when area < min_area (strictly) and, with keep_frame != 0, frame == 0.  Every pixel of a
 *   selected component gets the byte `value` (0..255) in mask_out, dense uint8 [n][h][w]; no other byte of mask_out is touched.  counts,
 *   64-bit [n][2], written whole by the call: {selected components, their pixels}.  min_area >= 0; 0 selects nothing.
 * runet_ccl_table: n_components, 64-bit [n] = the number of components of each image, exact even beyond capacity.  table, dense int32
 *   [n][capacity][8]: row k < min(capacity, n_components[i]) of image i describes the component of k-th smallest label as
 *   {label, area, x0, y0, x1, y1, frame, 0}, [x0, x1] x [y0, y1] the inclusive bounding box.  Rows from n_components[i] on, and everything
 *   past `capacity` rows, are not written.  capacity >= 0; with capacity == 0 only the count is made and table may be NULL.
 *   workspace: the roots before each chunk of 1024 pixels and every root's rank, 8-byte aligned. */
long runet_ccl_workspace_bytes(int n, int h, int w);
int runet_ccl_label_u8(const unsigned char* mask, int n, int h, int w, long row_stride, long image_stride, int invert, int connectivity, int* labels,
                       void* workspace, long workspace_bytes, void* stream);
int runet_ccl_areas(const int* labels, int n, int h, int w, int* areas, unsigned char* frame, void* stream);
int runet_ccl_filter_u8(const int* labels, const int* areas, const unsigned char* frame, int n, int h, int w, int min_area, int keep_frame,
                        int value, unsigned char* mask_out, long* counts, void* stream);
int runet_ccl_table(const int* labels, const int* areas, const unsigned char* frame, int n, int h, int w, int capacity, long* n_components,
                    int* table, void* workspace, long workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
