/*
 * hrviton_hip.h -- C ABI of the MI355X (gfx950) HR-VITON hot path.
 *
 * The reference (sangyun884/HR-VITON) is pure Python/PyTorch: it has no FFI of
 * its own, so the "plugin boundary" for the hot path is the set of torch ops
 * its modules dispatch.  Every entry point below replaces
 * one such dispatch (file:line into /root/reference cited per function) and is
 * what a ctypes / cffi / pybind stub on the reference side would bind
 * (INTEGRATION.md shows the stub).  Conventions:
 *
 *   - plain C: raw device pointers + sizes, no torch types, no C++ in the
 *     signatures.  `hrv_stream_t` is a `hipStream_t` passed as void*.
 *   - activations are NHWC fp32 (or bf16 where the name says so); a tensor is
 *     addressed as base[pixel * cstride + coff + c] so channel-concatenation and
 *     channel-slicing never need a copy.  Channel counts handed to the conv
 *     engine are multiples of 4 (callers zero-pad, e.g. 9 -> 12).
 *   - all memory is caller-owned; kernels borrow pointers for the duration of
 *     the launch on `stream`; no hidden allocation, no global state but the
 *     thread-local last-error string.
 *   - return value: 0 (HRV_OK) or a negative hrv_status; hrv_last_error() gives
 *     the message.  Nothing here ever falls back to a CPU path.
 */
#ifndef HRVITON_HIP_H
#define HRVITON_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* hrv_stream_t; /* hipStream_t */

enum hrv_status {
  HRV_OK = 0,
  HRV_ERR_ARG = -1,    /* bad shape / alignment / null pointer */
  HRV_ERR_LAUNCH = -2, /* hipLaunch / hipGetLastError failure */
  HRV_ERR_NODEV = -3   /* no gfx950 device */
};

enum hrv_act { HRV_ACT_NONE = 0, HRV_ACT_RELU = 1, HRV_ACT_LRELU = 2, HRV_ACT_TANH = 3 };

const char* hrv_version(void);
const char* hrv_last_error(void);
/* 0 if a gfx950 device is visible to the process. */
int hrv_device_check(void);
/* Persistent kernels (one block per CU holding most of its LDS: the SPADE gamma|beta kernel, the patch tiles, the thin and
 * weight-gradient kernels) size their grids to the CURRENT device's CU count (cached per device) minus ``k`` reserved CUs,
 * so that kernels which must run concurrently with them -- RCCL's collectives during a data-parallel backward (the
 * reference's DataParallelWithCallback reduction, train_generator.py:171-178) -- find free CUs instead of queueing behind
 * 40 us .. 1 ms blocks.  Default 0; the environment variable HRV_RESERVE_CUS sets the initial value.
 * hrv_persistent_cus(): the resulting grid size. */
int hrv_set_reserved_cus(int32_t k);
int hrv_persistent_cus(void);
/* Diagnostics only (tools/gb_bench.py, tools/patch_timeline.py): a device buffer of 8 x uint64 per tile, OWNED BY THE TOOL,
 * into which the persistent tile kernels write per-tile phase timestamps while it is set; (NULL, 0) switches it off.  A
 * launch with more tiles than the buffer holds does not log. */
int hrv_diag_set_tlog(void* buf, int64_t tiles);
/* The library's A/B and diagnostic switches (environment variables HRV_*) are read from the environment once per
 * name and cached, so no launch path calls getenv() after a name's first use.  A process that changes one of them while it runs
 * (tests/, tools/conv_bench.py) calls this to drop the cache. */
int hrv_diag_reload_env(void);

/* ------------------------------------------------------------------------
 * Convolution engine (implicit GEMM on fp32 MFMA, v_mfma_f32_32x32x2_f32).
 * Replaces every nn.Conv2d on the path: networks.py:171-198 (ResBlock
 * 3x3 s1/s2, 1x1), :63-93 (conv1/conv2/flow_conv/bottleneck);
 * network_generator.py:97-99,132-143,184-186,201 (SPADE / resblock / stem
 * convs) and :263-272 (4x4 s2 PatchGAN), with the surrounding
 * eval-BatchNorm / bias / residual / ReLU|LeakyReLU|tanh fused as an epilogue:
 *     out = act( acc * scale[c] + shift[c] + residual )
 * and torch.cat(..., 1) / nn.Upsample(nearest, x2) of the *inputs* folded into
 * the gather (several sources, optional half-resolution source).
 * ---------------------------------------------------------------------- */
#define HRV_MAX_SRC 4

typedef struct hrv_src {
  const void* ptr;  /* NHWC base */
  int32_t C;        /* channels taken from this source (multiple of 4)       */
  int32_t cstride;  /* channels per pixel in memory (multiple of 4)          */
  int32_t coff;     /* first channel (multiple of 4)                         */
  int32_t up_shift; /* 0: source is H x W; 1: source is (H/2) x (W/2), read through
                       a nearest x2 upsample (network_generator.py:203);
                       -k: source is (H<<k) x (W<<k), read through a nearest
                       1/2^k downsample (F.interpolate nearest, :164,222)    */
  int32_t pre_act;  /* must be HRV_ACT_NONE for the MFMA engine (activations are
                       fused into the producer's epilogue); LRELU(0.2) is
                       honoured by the naive cross-check only               */
  int32_t C_real;   /* channels that exist in the raw OIHW weight for this
                       source (<= C; 0 means C).  Only the naive cross-check
                       reads it; the packed weight already has zero rows.    */
} hrv_src_t;

/* SPADE epilogue (network_generator.py:101-122 + the LeakyReLU of :170-171): when
 * hrv_conv2d_t.spade is set the convolution is the fused conv_gamma||conv_beta
 * (128 -> 2C, 3x3) and the epilogue modulates the tensor being normalised:
 *     v   = x + noise_z[n,w,h] * noise_scale[c]
 *     out = act( (v - mean[n,c]) * rstd[n,c] * (1 + gamma) + beta )
 * w_packed holds 2*ceil32(C) output columns ordered in (gamma[32] | beta[32])
 * pairs per 32-channel group; `shift` holds the two biases in the same column
 * order; `scale`/`residual` are ignored; `Cout` is that column count; `out`
 * has C channels.  mean/rstd come from hrv_instnorm_stats_nhwc_f32. */
typedef struct hrv_spade_epi {
  const float* x;      /* NHWC, same pixels as out */
  int32_t x_cstride, x_coff;
  int32_t C;           /* channels (multiple of 4; pad channels are zero)     */
  int32_t _pad;
  const float* mean;   /* [N][C] */
  const float* rstd;   /* [N][C] */
  const float* noise_z;     /* [N][W][H] N(0,1) draw, layout of torch.randn(b,w,h,1)
                               (network_generator.py:104-107), or NULL        */
  const float* noise_scale; /* [C] or NULL */
  float* g1p_out;      /* training: (1 + gamma) is also stored here, NHWC [.,C] dense
                          (needed by hrv_spade_norm_bwd_nhwc_f32), or NULL          */
} hrv_spade_epi_t;

typedef struct hrv_conv2d {
  int32_t N, H, W;   /* conv input extent (after any folded upsample)        */
  int32_t Ho, Wo;    /* output extent                                        */
  int32_t KH, KW, stride, pad;
  int32_t nsrc;
  hrv_src_t src[HRV_MAX_SRC];
  const void* w_packed; /* from hrv_conv2d_pack_weight_f32 (device copy)     */
  const float* w_oihw;  /* device copy of the raw [Cout][Cin][KH][KW] weight;
                           only read by hrv_conv2d_naive_nhwc_f32            */
  int32_t Cout;
  int32_t tile_cfg;     /* from hrv_conv2d_pick_tile                         */
  const float* scale;   /* [Cout] or NULL (=1)                               */
  const float* shift;   /* [Cout] or NULL (=0)                               */
  const void* residual; /* NHWC, same pixels as out, or NULL                 */
  int32_t res_cstride, res_coff;
  int32_t act;          /* hrv_act                                           */
  float act_slope;      /* LeakyReLU negative slope                          */
  void* out;            /* NHWC                                              */
  int32_t out_cstride, out_coff;
  const hrv_spade_epi_t* spade; /* NULL: standard epilogue                   */
  int32_t out_up_shift; /* 1: `out` is (2*Ho) x (2*Wo) and every result is stored
                           to its 2x2 block -- the nn.Upsample(nearest, x2) that
                           follows each SPADEResBlock (network_generator.py:226-
                           241) fused into the producer's store; 0: plain      */
  int32_t _pad2;
  void* workspace;          /* optional scratch for split-K (small-M / large-K layers):   */
  int64_t workspace_bytes;  /* >= hrv_conv2d_workspace_bytes(d); NULL => run unsplit     */
  /* --- backward-pass extensions (all 0 for an ordinary forward convolution) --- */
  int32_t pad_w_plus1;  /* 0: horizontal padding = pad; else horizontal padding + 1        */
  int32_t free_extent;  /* 1: Ho/Wo are taken as given; taps outside the input read zeros  */
  int32_t out_step;     /* 2: row (n,h,w) is stored at (2h+out_off_h, 2w+out_off_w) of an
                           out_H x out_W tensor: one phase of a stride-2 data gradient     */
  int32_t out_off_h, out_off_w, out_H, out_W;
  int32_t res_mode;     /* 0: epilogue adds `residual`; 1: multiplies by the activation
                           derivative (residual > 0 ? 1 : act_slope) -- LeakyReLU/ReLU
                           backward fused into the data-gradient convolution             */
  int32_t mixed_flags;  /* hrv_conv2d_nhwc_bf16 only: bit0 = `out` is fp32, bit1 = `residual` is fp32,
                           bit2 = the SPADE `x` is fp32 (tensors that feed an InstanceNorm stay fp32),
                           bit3 = the conv SOURCES are fp32 and are rounded to bf16 while staged
                           (mixed-precision training; needs a 128-byte-row tile, cfg 8/9) */
  int32_t _pad3;
} hrv_conv2d_t;

/* Tile configuration for (M = N*Ho*Wo output pixels, Cout): returns cfg id. */
int hrv_conv2d_pick_tile(int64_t M, int32_t Cout);
/* BN (output-channel tile) / BM (pixel tile) of a cfg; <0 if cfg is invalid. */
int hrv_conv2d_tile_bn(int32_t tile_cfg);
int hrv_conv2d_tile_bm(int32_t tile_cfg);
/* Bytes per packed K-tile row of the bf16 engine for a cfg (64 = 32 k-values, 128 = 64 k-values); <0 if invalid. */
int hrv_conv2d_tile_row_bytes(int32_t tile_cfg);
/* Number of floats of the packed weight for this layer. */
int64_t hrv_conv2d_packed_elems(int32_t Cout, int32_t KH, int32_t KW, int32_t nsrc,
                                const int32_t* srcC, int32_t tile_cfg);
/* HOST function: repack w[Cout][sum(srcC_real)][KH][KW] (torch layout) into the
 * K-tiled layout the MFMA kernel streams:  [kt][CoutPad][16] with
 * kt = ((kh*KW + kw) * chunks_total + chunk) and chunk running over the
 * sources' 16-channel groups.  srcC[i] are the padded per-source channel
 * counts used by the kernel (multiples of 4), srcC_real[i] the channels that
 * exist in w (<= srcC[i]); padded rows are zero. */
int hrv_conv2d_pack_weight_f32(const float* w_oihw, int32_t Cout, int32_t KH, int32_t KW, int32_t nsrc,
                               const int32_t* srcC, const int32_t* srcC_real, int32_t tile_cfg,
                               float* out);
/* ---- training side (conv_bwd.hip) ---------------------------------------
 * Device-side weight packing (weights change every optimiser step).  mode 0: the
 * forward layout of hrv_conv2d_pack_weight_f32; mode 1: the stride-1 data gradient
 * (rows = Cin, k over Cout, taps flipped; run the engine on dY with pad K-1-pad);
 * mode 2: one phase (phase_a, phase_b) of the stride-2 data gradient
 * (dX[2h'+a] = sum_j dY[h'+j-pad_p] W[a+pad-2(j-pad_p)]).  `wscale` multiplies
 * every weight; if sigma_dev != NULL the weights are also divided by the device
 * scalar sigma_dev[0] (spectral norm, no host sync).  out_geom[8] = {KHp, KWp, pad_h, pad_w,
 * rows, rows_pad, chunks_total, packed elems}; out_dev must hold that many floats
 * (<= KH*KW*chunks*rows_pad*16).
 * Weight gradient of one source of a (possibly concatenated) input:
 *   dW[co][ci_base+ci][kh][kw] (+)= sum_p dY[p][co] * X[p shifted by (kh,kw)][ci]
 * MFMA GEMM over pixel slabs + fixed-order reduction (deterministic).
 * colsum: out[c] (+)= sum_p x[p][c]  (bias gradient).
 * ---------------------------------------------------------------------- */
int hrv_conv2d_pack_weight_dev_f32(const float* w_oihw_dev, int32_t Cout, int32_t KH, int32_t KW, int32_t nsrc,
                                   const int32_t* srcC, const int32_t* srcC_real, int32_t tile_cfg, int32_t mode,
                                   int32_t stride, int32_t pad, int32_t phase_a, int32_t phase_b, float wscale,
                                   const float* sigma_dev, float* out_dev, int32_t* out_geom, hrv_stream_t stream);
/* Same packing, rounded to bf16, for the bf16 matrix-core engine (hrv_conv2d_nhwc_bf16): rows of 64 k-values
 * for the 128-byte-row tiles (tile_cfg 8/9), 32 otherwise.  Used by mixed-precision training, where the
 * activations stay fp32 in HBM (hrv_conv2d_t.mixed_flags bit 3) and only the MFMA operands are bf16. */
int hrv_conv2d_pack_weight_dev_bf16(const float* w_oihw_dev, int32_t Cout, int32_t KH, int32_t KW, int32_t nsrc,
                                    const int32_t* srcC, const int32_t* srcC_real, int32_t tile_cfg, int32_t mode,
                                    int32_t stride, int32_t pad, int32_t phase_a, int32_t phase_b, float wscale,
                                    const float* sigma_dev, uint16_t* out_dev, int32_t* out_geom, hrv_stream_t stream);
/* The same packing for a weight PAIR -- SPADE conv_gamma / conv_beta (network_generator.py:93-118), both
 * [rows_each][Cin][KH][KW] -- without materialising the combined matrix.  pair_mode 1: forward (mode 0), virtual
 * Cout = 64*ceil(rows_each/32) rows interleaved (gamma32 | beta32), the column order of the fused modulate epilogue;
 * pair_mode 2: stride-1 data gradient (mode 1) over dY = [dgamma | dbeta], Cout = 2 * (channels per half). */
int hrv_conv2d_pack_weight_pair_dev(const float* w_a_dev, const float* w_b_dev, int32_t rows_each, int32_t pair_mode,
                                    int32_t Cout, int32_t KH, int32_t KW, int32_t nsrc, const int32_t* srcC,
                                    const int32_t* srcC_real, int32_t tile_cfg, int32_t mode, int32_t pad, int32_t as_bf16,
                                    void* out_dev, int32_t* out_geom, hrv_stream_t stream);
/* Batched form of the three packs above: every weight of a network re-packed by ONE launch per training step (the
 * reference re-derives nothing -- cuDNN reads OIHW -- so this replaces ~180 small launches of this library's own).
 * hrv_conv2d_pack_weight_record fills a host record (hrv_conv2d_pack_record_bytes() bytes) for one pack -- same argument
 * meaning; as_bf16 selects the bf16 form; w2_dev / pair_mode / rows_each describe a pair, else null / 0 / 0 -- and
 * returns its geometry and block count; the caller keeps the records in a device array, their block prefix sums in
 * first_block_dev[n + 1], and launches hrv_conv2d_pack_weight_multi whenever the weights changed. */
int32_t hrv_conv2d_pack_record_bytes(void);
int hrv_conv2d_pack_weight_record(const float* w_oihw_dev, int32_t Cout, int32_t KH, int32_t KW, int32_t nsrc,
                                  const int32_t* srcC, const int32_t* srcC_real, int32_t tile_cfg, int32_t mode,
                                  int32_t stride, int32_t pad, int32_t phase_a, int32_t phase_b, float wscale,
                                  const float* sigma_dev, int32_t as_bf16, const float* w2_dev, int32_t pair_mode,
                                  int32_t rows_each, void* out_dev, int32_t* out_geom, void* record_host, int32_t* blocks);
int hrv_conv2d_pack_weight_multi(const void* records_dev, const int32_t* first_block_dev, int32_t n, int32_t blocks,
                                 hrv_stream_t stream);
int64_t hrv_conv2d_wgrad_workspace_bytes(int32_t Cout, int32_t CinTot, int32_t KH, int32_t KW, int64_t P);
/* dy / x: fp32 elements, or bf16 where storage_flags says so -- bit0: `dy` points at bf16 elements, bit1: `x` does (counts in
 * elements, multiples of 4).  Tensors that only matrix cores read are kept in bf16 by the mixed-precision training plan (same MMA
 * operand bits, half the bytes).  Supported: 0, 2 (x), 3 (both); bf16 storage needs mma_bf16.
 * mma_bf16 1: the operands are rounded to bf16 while staged and multiplied on v_mfma_f32_32x32x16_bf16 (fp32 accumulate) -- the
 * weight gradient of mixed-precision training; 0: fp32 MFMA.
 * dbias (optional, [Cout]): the bias gradient sum_pixels dY[:, co], fused as one extra "ones" column of the same
 * MFMA reduction (no second pass over dY; deterministic).  Pass it with the FIRST source of a concatenation only. */
typedef struct hrv_conv2d_wgrad {
  const void* dy;       /* NHWC [N][Ho][Wo], Cout channels at dy_coff of dy_cstride                       */
  int32_t dy_cstride, dy_coff, Cout;
  int32_t x_C;          /* channels taken from x (padded: a multiple of 4)                               */
  const void* x;        /* NHWC source, read through x_up_shift as hrv_src_t.up_shift                    */
  int32_t x_cstride, x_coff, x_up_shift;
  int32_t x_C_real;     /* channels of x that exist in the weight (<= x_C)                               */
  int32_t ci_base, CinTot; /* dW[:, ci_base : ci_base + x_C_real] of a weight with CinTot input channels */
  int32_t N, H, W;      /* conv input extent (after any folded resampling of x)                          */
  int32_t Ho, Wo;       /* extent of dy                                                                  */
  int32_t KH, KW, stride, pad;
  int32_t mma_bf16, storage_flags;
  int32_t _pad;
  float* workspace;         /* >= hrv_conv2d_wgrad_workspace_bytes(Cout, CinTot, KH, KW, N*Ho*Wo)        */
  int64_t workspace_bytes;
  float* dw_oihw;       /* [Cout][CinTot][KH][KW] fp32                                                   */
  float* dbias;         /* [Cout] or NULL                                                                */
  int32_t accumulate, dbias_accumulate;     /* 1: += into dw_oihw / dbias                                */
} hrv_conv2d_wgrad_t;
/* The kernel that serves a descriptor.  The LDS-DMA kernels (wgrad_tr.hip: stride-1 'same' layers, wgrad_s2.hip: PatchGAN's 4x4
 * stride-2 pad-2 layers; both operands bf16-stored, any output width) go first, then the generic quad-staged kernels. */
enum hrv_wgrad_route {
  HRV_WGRAD_F32 = 0,    /* conv_wgrad_mfma_kernel                                                         */
  HRV_WGRAD_BF16 = 1,   /* conv_wgrad_bf16_kernel: needs Wo % 4 == 0 at launch (hrv_pad_width_nhwc_bf16)  */
  HRV_WGRAD_S2 = 2,     /* conv_wgrad_s2_kernel                                                           */
  HRV_WGRAD_TR = 3      /* conv_wgrad_tr_kernel: HRV_WGRAD_TR + its shape class 0..8                      */
};
/* HOST function, launches nothing: the hrv_wgrad_route hrv_conv2d_wgrad takes for `d`, from the very code that launches (the
 * HRV_WGRAD_TR / HRV_WGRAD_TR_MIN_PIX / HRV_WGRAD_S2 switches, the pixel, width, granule and slab-extent limits included), or
 * HRV_ERR_ARG for a storage form that is not built.  Reads metadata only: the pointers of `d` may be NULL. */
int hrv_conv2d_wgrad_route(const hrv_conv2d_wgrad_t* d);
int hrv_conv2d_wgrad(const hrv_conv2d_wgrad_t* d, hrv_stream_t stream);
int hrv_colsum_nhwc_f32(const float* x, int64_t P, int32_t C, int32_t cstride, int32_t coff, float* workspace,
                        int64_t workspace_bytes, float* out, int32_t accumulate, hrv_stream_t stream);

/* ---- training side, HBM-bound kernels (norm_bwd.hip, train.hip) -------------------------
 * SPADE / InstanceNorm backward (network_generator.py:101-122 + LeakyReLU :170-171;
 * PatchGAN IN+LeakyReLU :263-272) for
 *     v = x + noise_z*noise_scale;  nh = (v - mean)*rstd;  out = act(nh*g1p + beta)
 * given dout:  dpre = dout*act'(out); dnh = dpre*g1p; dgamma = dpre*nh; dbeta = dpre;
 *     dx = rstd*(dnh - mean_hw(dnh) - nh*mean_hw(dnh*nh));  dnoise_scale = sum dx*z.
 * g1p = 1+gamma (NULL: plain InstanceNorm, dgb must be NULL); dgb receives
 * [dgamma | dbeta] (2C channels); dnh is a C-channel scratch/output tensor.
 * workspace: hrv_norm_bwd_workspace_elems floats.  Deterministic (2-stage sums).
 * dbeta in place: when `dout` IS the dbeta half of `dgb` (same base pointer, same pixel stride, dout_coff == dgb_coff + C,
 * same storage type, act == NONE -- the data gradient that produced dout wrote it there with the activation derivative
 * applied in its own epilogue) the kernel reads it from there and does not store dbeta again. */
typedef struct hrv_norm_bwd {
  int32_t N, H, W, C;
  const float* x;     int32_t x_cstride, x_coff;
  const float* noise_z; const float* noise_scale;      /* nullable (together) */
  const float* mean;  const float* rstd;               /* [N][C] */
  const float* out;   int32_t out_cstride, out_coff;   /* activation output (its mask) */
  const float* g1p;   int32_t g1p_cstride, g1p_coff;   /* 1+gamma, nullable */
  const float* dout;  int32_t dout_cstride, dout_coff;
  float* dnh;         int32_t dnh_cstride, dnh_coff;
  float* dgb;         int32_t dgb_cstride, dgb_coff;   /* nullable */
  float* dx;          int32_t dx_cstride, dx_coff;
  int32_t dx_accumulate;                               /* 1: dx += ... */
  int32_t act;        float act_slope;
  int32_t dns_accumulate;
  float* dnoise_scale;                                 /* [C], nullable */
  float* workspace;
  int32_t dgb_bf16;   /* 1: `dgb` is stored as bf16 (element strides/offsets): a tensor only matrix cores read */
  int32_t out_bf16;   /* 1: `out` is stored as bf16 (only its sign is used here)                              */
  int32_t dx_bf16;    /* 1: `dx` is stored as bf16 (no accumulate): the gradient of a convolution output that only
                       *    that convolution's weight / data gradient (matrix cores) read                          */
  int32_t g1p_bf16;   /* 1: `g1p` is stored as bf16 (written by hrv_spade_gb_bf16; this kernel is its only reader) */
  int32_t dnh_bf16;   /* 1: the stage-1 -> stage-2 intermediate `dnh` is stored as bf16 (mixed precision: half its bytes) */
  int32_t dout_bf16;  /* 1: `dout` is stored as bf16 (mixed precision: the data gradient of a bf16-stored SPADE output, as
                       * autocast hands the gradient of a half-precision convolution input back in half precision) */
  /* x = cat(nearest_up2(lo), hi) along channels, never materialised (x_up_channels > 0; SPADEGenerator.up + the resized-input
   * concatenation, network_generator.py:203,226-242): channels [0, x_up_channels) are read from `x` = lo [N][H/2][W/2][x_cstride]
   * at (h >> 1, w >> 1), the remaining C - x_up_channels from `x2` = hi [N][H][W][x2_cstride] */
  int32_t x_up_channels;
  const float* x2;    int32_t x2_cstride, x2_coff;
} hrv_norm_bwd_t;
int64_t hrv_norm_bwd_workspace_elems(int32_t N, int32_t H, int32_t W, int32_t C);

/* Thin convolution (thin_conv.hip): 3x3 / 1x1 stride-1 'same' nn.Conv2d with <= 96 channels on either side over a
 * bf16-STORED NHWC source, forward (mode 0) or data gradient (mode 1: `src` is dY with Cout channels, the result has
 * Cin columns, taps flipped) -- SPADEResBlock.conv_0 / conv_1 / conv_s at 1024x768 and conv_img
 * (network_generator.py:141-143,201) in mixed-precision training.  `w_oihw` is the fp32 parameter on the device
 * (weight_orig for spectral-norm layers; the kernel multiplies it by wscale / sigma[0]).
 * out = act((conv + shift[c]) (+ residual | * act'(residual) for res_mode 1)), fp32 or bf16.
 * hrv_thin_conv_supported() says whether a (kernel, source-channel, column) combination is instantiated. */
typedef struct {
  const void* src; int32_t N, H, W, src_channels, src_cstride, src_coff;
  const float* w_oihw; int32_t Cout, Cin, KH, KW; const float* sigma; float wscale;
  int32_t mode;
  const float* shift;
  const void* residual; int32_t res_cstride, res_coff, res_bf16, res_mode;
  int32_t act; float act_slope;
  void* out; int32_t out_cstride, out_coff, out_bf16;
} hrv_thin_conv_t;
int hrv_thin_conv_supported(int32_t KH, int32_t KW, int32_t src_channels, int32_t out_columns);
int hrv_thin_conv_bf16(const hrv_thin_conv_t* d, hrv_stream_t stream);
int hrv_spade_norm_bwd_nhwc_f32(const hrv_norm_bwd_t* d, hrv_stream_t stream);
/* Two normalisations of the SAME x (norm_0 and norm_s of a learned-shortcut SPADEResBlock, network_generator.py:158-166) in one
 * pass per stage: x is read once, a->dx <- dx_a + dx_b is written once (b->dx is ignored); everything else per descriptor.
 * Bit-identical to hrv_spade_norm_bwd_nhwc_f32(a) followed by (b with dx = a->dx, dx_accumulate = 1). */
int hrv_spade_norm_bwd2_nhwc_f32(const hrv_norm_bwd_t* a, const hrv_norm_bwd_t* b, hrv_stream_t stream);
/* Compile-time instances.  Both entry points above pick, per stage, a kernel compiled for the descriptor's storage form (which
 * operands are bf16, whether there is noise, an activation, 1 + gamma, [dgamma | dbeta], dbeta in place, an up-sampled source,
 * how dx is stored) where that form is in the library's table, and the generic run-time kernel otherwise or when
 * HRV_NORM_BWD_GENERIC=1; results are bit-identical either way.
 * hrv_diag_norm_bwd_instances: the table, one "<single|pair>.<stage1|stage2> <form>" line per kernel.
 * hrv_diag_norm_bwd_route(a, b or NULL): bit 0 = stage 1 of this descriptor (pair) runs on an instance, bit 1 = stage 2; < 0: the
 *   descriptor is refused.
 * hrv_spade_norm_bwd2_supported(a, b): 1 where the one-pass pair is the faster form for these two descriptors (both stages on an
 *   instance; measured per level), 0 where two sequential calls are, or the pair is not valid. */
const char* hrv_diag_norm_bwd_instances(void);
int hrv_diag_norm_bwd_route(const hrv_norm_bwd_t* a, const hrv_norm_bwd_t* b);
int hrv_spade_norm_bwd2_supported(const hrv_norm_bwd_t* a, const hrv_norm_bwd_t* b);
/* Loss value + gradient in one pass.  mode 0: L1 |a-b| (feature matching / VGG,
 * train_generator.py:300-312); 1: hinge-D fake max(1+a,0); 2: hinge-D real max(1-a,0);
 * 3: -a (generator hinge) (network_generator.py:365-376); 4: (a-b)^2 (LSGAN, networks.py:258-299).
 * loss_out[0] (+)= lscale*sum(l);  grad[i] = gscale*dl/da (grad may be NULL).
 * workspace: 1024 floats. */
int hrv_loss_f32(const float* a, const float* b, int64_t n, int32_t mode, float lscale, float gscale, float* grad,
                 float* workspace, float* loss_out, int32_t accumulate, hrv_stream_t stream);
int hrv_loss_bf16in_f32(const uint16_t* a, const uint16_t* b, int64_t n, int32_t mode, float lscale, float gscale, float* grad,
                        float* workspace, float* loss_out, int32_t accumulate, hrv_stream_t stream);
/* tanh backward through its output: out = dy*(1-y*y) (network_generator.py:245);
 * add_slice: out[.., out_coff:+C] (+)= a[.., a_coff:+C]  (gradient accumulation / channel split). */
/* x *= s_host * (s_dev ? s_dev[0] : 1): applies an upstream (device-resident) loss-gradient scalar. */
int hrv_scale_f32(float* x, int64_t n, float s_host, const float* s_dev, hrv_stream_t stream);
/* d *= act'(y) in place (ReLU / LeakyReLU derivative through the activation output y). */
int hrv_act_bwd_nhwc_f32(float* d, int32_t d_cstride, int32_t d_coff, const float* y, int32_t y_cstride, int32_t y_coff,
                         int32_t C, int64_t npix, int32_t act, float act_slope, hrv_stream_t stream);
int hrv_tanh_bwd_f32(const float* dy, const float* y, int64_t n, float* out, hrv_stream_t stream);
int hrv_add_slice_nhwc_f32(const float* a, int32_t a_cstride, int32_t a_coff, float* out, int32_t out_cstride,
                           int32_t out_coff, int32_t C, int64_t npix, int32_t accumulate, hrv_stream_t stream);
/* nn.Upsample(nearest, x2) backward: dlo (+)= 2x2 block sums of dhi.  accumulate: 0 write, 1 add, 2 write as bf16
 * (lo_cstride / lo_coff then count bf16 elements). */
int hrv_downsum2x2_nhwc_f32(const float* dhi, int32_t N, int32_t Hl, int32_t Wl, int32_t C, int32_t hi_cstride,
                            int32_t hi_coff, float* dlo, int32_t lo_cstride, int32_t lo_coff, int32_t accumulate,
                            hrv_stream_t stream);
int hrv_avgpool3x3s2_bwd_nhwc_f32(const float* dy, int32_t N, int32_t H, int32_t W, int32_t C, int32_t dy_cstride,
                                  int32_t dy_coff, float* dx, int32_t dx_cstride, int32_t dx_coff, int32_t accumulate,
                                  hrv_stream_t stream);
/* VGG19 2x2/2 max pool (networks.py:201-232 via torchvision cfg 'E'), dense NHWC. */
int hrv_maxpool2x2_nhwc_f32(const float* x, int32_t N, int32_t H, int32_t W, int32_t C, float* y, hrv_stream_t stream);
int hrv_maxpool2x2_bwd_nhwc_f32(const float* x, const float* dy, int32_t N, int32_t H, int32_t W, int32_t C, float* dx,
                                hrv_stream_t stream);
/* ... with the ReLU derivative of the pooled tensor fused (x = ReLU(pre); dx is the gradient w.r.t. pre). */
int hrv_maxpool2x2_bwd_relu_nhwc_f32(const float* x, const float* dy, int32_t N, int32_t H, int32_t W, int32_t C, float* dx,
                                     hrv_stream_t stream);
/* bf16-stored activations (mixed-precision VGG19: matrix cores, pools and the L1 taps are their only readers;
 * forward bf16 -> bf16 for NON-NEGATIVE inputs (ReLU outputs: integer max of the stored patterns, exact); backward with
 * bf16 x, fp32 dy / dx; loss over bf16 a, b. */
int hrv_maxpool2x2_nhwc_bf16(const uint16_t* x, int32_t N, int32_t H, int32_t W, int32_t C, uint16_t* y, hrv_stream_t stream);
/* mixed-precision VGG19 BACKWARD keeps its gradient tensors in bf16 too (their readers are the data-gradient matrix cores,
 * the pool routing and these sums): pool backward over bf16 x / dy / dx; out (+)= a over bf16 tensors (fp32 sum, one
 * rounding); hrv_loss_bf16in_f32 with mode | 32 stores its gradient as bf16 (`grad` then points at bf16 elements). */
int hrv_maxpool2x2_bwd_relu_nhwc_bf16(const uint16_t* x, const uint16_t* dy, int32_t N, int32_t H, int32_t W, int32_t C,
                                      uint16_t* dx, hrv_stream_t stream);
int hrv_add_slice_nhwc_bf16(const uint16_t* a, int32_t a_cstride, int32_t a_coff, uint16_t* out, int32_t out_cstride,
                            int32_t out_coff, int32_t C, int64_t npix, int32_t accumulate, hrv_stream_t stream);
int hrv_maxpool2x2_bwd_relu_nhwc_xbf16(const uint16_t* x, const float* dy, int32_t N, int32_t H, int32_t W, int32_t C,
                                       float* dx, hrv_stream_t stream);
/* torch.optim.Adam step over one flat buffer (train_generator.py:154-157,322,360);
 * g is multiplied by grad_scale first (1/world_size after a sum all-reduce). */
int hrv_adam_f32(float* w, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                 float weight_decay, int32_t step, float grad_scale, hrv_stream_t stream);
/* The same update with its step-dependent scalars on the device, for a hipGraph-captured training iteration (a replay must
 * not freeze the step count or the learning rate into launch arguments): hrv_adam_hyper_f32 increments step_dev[0] and
 * writes hyper_dev[3] = {lr_dev[0], 1 - beta1^t, sqrt(1 - beta2^t)}; hrv_adam_dev_f32 reads them. */
int hrv_adam_hyper_f32(int32_t* step_dev, const float* lr_dev, float beta1, float beta2, float* hyper_dev, hrv_stream_t stream);
int hrv_adam_dev_f32(float* w, const float* g, float* m, float* v, int64_t n, const float* hyper_dev, float beta1, float beta2,
                     float eps, float weight_decay, float grad_scale, hrv_stream_t stream);
/* Guarded Adam step: gradient norm, clipping and the skip of a non-finite step, decided ON THE DEVICE (no host read, capturable).
 *
 * hrv_grad_sumsq_f32: one pass over g[0, n) (any 4-byte-aligned pointer, any n >= 1; nothing outside [0, n) is read).  Slot s of
 * the hrv_grad_guard_slots() slots receives part[s] = sum of (double)g[i]^2 over its elements and cnt[s] = how many of them are
 * non-finite (exponent field all ones).  The slot count is a compile-time constant of the library, the element -> slot rule and
 * every summation order are fixed and no atomics are used: the same buffer gives the same bits in every run and on every card.
 *
 * hrv_grad_guard_finalize: one block sums the slots in fixed order and fills the guard record, HRV_GUARD_WORDS 32-bit words:
 *   [HRV_GUARD_NORM]      f32  grad_scale * sqrt(sumsq), rounded once to fp32
 *   [HRV_GUARD_SCALE]     f32  min(1, max_norm / (norm + 1e-6)) in fp32 (torch.nn.utils.clip_grad_norm_; a NaN norm gives NaN, as
 *                              there); exactly 1.0f when clipping is off (max_norm <= 0)
 *   [HRV_GUARD_APPLY]     i32  0 when skip_nonfinite is set and (the count is non-zero or norm is not finite in fp32), else 1
 *   [HRV_GUARD_NONFINITE] i32  this step's count of non-finite elements
 *   [HRV_GUARD_STEPS]     i32  running total: steps seen
 *   [HRV_GUARD_SKIPPED]   i32  running total: steps with apply == 0
 *   [HRV_GUARD_CLIPPED]   i32  running total: applied steps with scale < 1
 *   [7]                        reserved (0)
 *   [HRV_GUARD_SUMSQ, +1] f64  the un-scaled sum of squares
 *   [10 .. 15]                 reserved
 * The three totals continue from what the record holds: zero it once before the first step.
 * hrv_grad_guard_finalize_hyper additionally does the work of hrv_adam_hyper_f32, but ONLY when apply == 1: a skipped step leaves
 * step_dev and hyper_dev alone, so it does not advance the bias correction.
 *
 * hrv_adam_guarded_f32 / hrv_adam_dev_guarded_f32: hrv_adam_f32 / hrv_adam_dev_f32 reading the record.  apply == 0: the launch
 * touches nothing.  Otherwise the gradient is (g * grad_scale) * scale; with scale == 1.0f the result has the bits of the plain
 * kernel. */
#define HRV_GUARD_NORM 0
#define HRV_GUARD_SCALE 1
#define HRV_GUARD_APPLY 2
#define HRV_GUARD_NONFINITE 3
#define HRV_GUARD_STEPS 4
#define HRV_GUARD_SKIPPED 5
#define HRV_GUARD_CLIPPED 6
#define HRV_GUARD_SUMSQ 8
#define HRV_GUARD_WORDS 16
int hrv_grad_guard_slots(void);
int hrv_grad_sumsq_f32(const float* g, int64_t n, double* part, int32_t* cnt, hrv_stream_t stream);
int hrv_grad_guard_finalize(const double* part, const int32_t* cnt, float grad_scale, float max_norm, int32_t skip_nonfinite,
                            int32_t* record, hrv_stream_t stream);
int hrv_grad_guard_finalize_hyper(const double* part, const int32_t* cnt, float grad_scale, float max_norm, int32_t skip_nonfinite,
                                  int32_t* record, int32_t* step_dev, const float* lr_dev, float beta1, float beta2,
                                  float* hyper_dev, hrv_stream_t stream);
int hrv_adam_guarded_f32(float* w, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                         float weight_decay, int32_t step, float grad_scale, const int32_t* record, hrv_stream_t stream);
int hrv_adam_dev_guarded_f32(float* w, const float* g, float* m, float* v, int64_t n, const float* hyper_dev, float beta1,
                             float beta2, float eps, float weight_decay, float grad_scale, const int32_t* record,
                             hrv_stream_t stream);
/* The four Adam launches above, each also keeping an exponential moving average ``ema`` of the weights (one more buffer of n
 * floats, read and written once: 36 bytes per element).  Per element, in fp32:
 *   w', m', v' = what the launch of the same name without _ema writes for the same arguments, bit for bit
 *   d   = warmup ? fminf(decay, (1 + t) / (10 + t)) : decay      t = the step count of this launch, as float
 *   omd = 1.f - d
 *   e'  = omd == 1.f ? w' : fmaf(omd, w' - e, e)                  (w' - e rounded to fp32 first)
 * 0 <= decay < 1.  t is ``step`` in the host-count variants; the device-count variants read step_dev[0], which hrv_adam_hyper_f32 /
 * hrv_grad_guard_finalize_hyper have already advanced for an applied step.  A guarded launch with apply == 0 leaves ema alone, like
 * w, m and v.  Any n >= 1 and any 4-byte-aligned pointers; with all five pointers on 16-byte boundaries a thread moves 16 bytes of
 * each array per trip, otherwise the whole launch moves 4.
 * hrv_swap_f32 exchanges a[0, n) and b[0, n) in place in one pass, no temporary (the buffers must not overlap); the same
 * alignment rule. */
int hrv_adam_ema_f32(float* w, const float* g, float* m, float* v, float* ema, int64_t n, float lr, float beta1, float beta2,
                     float eps, float weight_decay, int32_t step, float grad_scale, float decay, int32_t warmup, hrv_stream_t stream);
int hrv_adam_dev_ema_f32(float* w, const float* g, float* m, float* v, float* ema, int64_t n, const float* hyper_dev, float beta1,
                         float beta2, float eps, float weight_decay, float grad_scale, float decay, int32_t warmup,
                         const int32_t* step_dev, hrv_stream_t stream);
int hrv_adam_guarded_ema_f32(float* w, const float* g, float* m, float* v, float* ema, int64_t n, float lr, float beta1, float beta2,
                             float eps, float weight_decay, int32_t step, float grad_scale, const int32_t* record, float decay,
                             int32_t warmup, hrv_stream_t stream);
int hrv_adam_dev_guarded_ema_f32(float* w, const float* g, float* m, float* v, float* ema, int64_t n, const float* hyper_dev,
                                 float beta1, float beta2, float eps, float weight_decay, float grad_scale, const int32_t* record,
                                 float decay, int32_t warmup, const int32_t* step_dev, hrv_stream_t stream);
int hrv_swap_f32(float* a, float* b, int64_t n, hrv_stream_t stream);
/* Per-parameter statistics of an optimizer's flat buffers: one segmented reduction, read-only, two launches, no host read, no
 * atomics (capturable).  A span is one parameter's run of elements; the caller cuts every span into PIECES of at most
 * hrv_span_stats_piece() elements (a compile-time constant of the library), no piece crossing a span, a span's pieces consecutive.
 *
 * hrv_span_stats_f32: pieces[p] = {first element, length in 1 .. PIECE} (device memory, 8-byte aligned).  One block per piece reads
 * g, w and, where given, m and v (both or neither) over exactly the piece's elements -- nothing outside a piece is read -- and
 * writes part[p], HRV_SPAN_WORDS words laid out like a record, with plain stores.  Any 4-byte-aligned base pointers, any offsets:
 * where all arrays read share the position of a piece's first element inside 16 bytes a thread moves 16 bytes of each per trip
 * between a scalar head and tail, otherwise the piece is read element by element.  Per element, x standing for g, w and u:
 *   non-finite (exponent field all ones): counted and LEFT OUT of sum and maximum; finite: sumsq += (double)x * (double)x,
 *   maxabs = max(maxabs, fabsf(x)); for g, elements equal to +-0 are counted as well
 *   u = m / (sqrtf(v) / bc2_sqrt + eps) in fp32, every operation rounded on its own: the direction of the Adam update the moments
 *   stand for (hrv_adam_f32 forms mi / denom like this); an element whose m, v or u is non-finite counts in u_nonfinite
 *   bc2_sqrt is hyper_dev[2] where hyper_dev is given (hrv_adam_hyper_f32's output), else the scalar argument
 * The piece table alone decides every summation order (per thread over its trips in turn, then its head and tail elements, a
 * 64-lane shuffle tree, the block's waves in order): the same buffers give the same bits in every run, on every card and grid.
 *
 * hrv_span_stats_finalize: span s owns part[span_first[s] .. span_first[s + 1]); one wave per span adds them (lane l the
 * partials l, l + 64, ... in turn, then the shuffle tree) and writes records[s], HRV_SPAN_WORDS 32-bit words:
 *   [HRV_SPAN_G_SUMSQ, +1] f64   [HRV_SPAN_W_SUMSQ, +1] f64   [HRV_SPAN_U_SUMSQ, +1] f64 (0 without m / v)      un-scaled
 *   [HRV_SPAN_G_MAXABS] f32      [HRV_SPAN_W_MAXABS] f32      [HRV_SPAN_U_MAXABS] f32
 *   [HRV_SPAN_G_NONFINITE] i32   [HRV_SPAN_W_NONFINITE] i32   [HRV_SPAN_U_NONFINITE] i32   [HRV_SPAN_G_ZEROS] i32
 *   [13 .. 15] reserved, 0 */
#define HRV_SPAN_G_SUMSQ 0
#define HRV_SPAN_W_SUMSQ 2
#define HRV_SPAN_U_SUMSQ 4
#define HRV_SPAN_G_MAXABS 6
#define HRV_SPAN_W_MAXABS 7
#define HRV_SPAN_U_MAXABS 8
#define HRV_SPAN_G_NONFINITE 9
#define HRV_SPAN_W_NONFINITE 10
#define HRV_SPAN_U_NONFINITE 11
#define HRV_SPAN_G_ZEROS 12
#define HRV_SPAN_WORDS 16
int hrv_span_stats_piece(void);
int hrv_span_stats_f32(const float* g, const float* w, const float* m, const float* v, const int64_t* pieces, int32_t n_pieces,
                       const float* hyper_dev, float bc2_sqrt, float eps, void* part, hrv_stream_t stream);
int hrv_span_stats_finalize(const void* part, const int32_t* span_first, int32_t n_spans, int32_t* records, hrv_stream_t stream);
/* torch spectral_norm (SpectralNorm.compute_weight): `power_iterations` rounds of
 * v<-normalize(W^T u), u<-normalize(W v) in place (eps 1e-12), then sigma = u.(W v).
 * W is [R][K] = weight_orig.reshape(Cout,-1); wv_scratch holds R floats.
 * bwd: dW_orig (+)= (G - <G,W_orig>/sigma * u v^T)/sigma; workspace 1024 floats. */
int hrv_spectral_norm_f32(const float* w, int32_t R, int32_t K, float* u, float* v, int32_t power_iterations, float eps,
                          float* wv_scratch, float* sigma_out, hrv_stream_t stream);
int hrv_spectral_norm_bwd_f32(const float* G, const float* w_orig, const float* u, const float* v, const float* sigma,
                              int32_t R, int32_t K, float* workspace, float* dw_orig, int32_t accumulate,
                              hrv_stream_t stream);
/* Per-step parameter staging of a SPADE norm / block, one launch each:
 *  vec_prep: bias of the fused gamma|beta convolution in its interleaved column order (64*ceil(C/32) floats) and the
 *            noise scale zero-padded to ceil4(C);
 *  shared_taps_prep: conv_shared (label_nc=c -> hid, 3x3) of the n <= 4 norms of a block as ONE 1x1 weight
 *            wt[n*hid][9*cp] over the tap-expanded label map (tap-major, cp channels per tap) + concatenated bias;
 *  shared_taps_grad: the inverse map of that weight's gradient into the n conv_shared weight / bias gradients. */
int hrv_spade_vec_prep_f32(const float* gamma_bias, const float* beta_bias, const float* noise_scale, int32_t C,
                           float* bias_interleaved, float* noise_scale_padded, hrv_stream_t stream);
/* ... of n <= 32 norms in one launch: job i writes its interleaved bias at bias_interleaved_all + off_bias[i] ((C[i] + 31) / 32 * 64
 * floats) and its padded noise scale at noise_scale_padded_all + off_noise[i] (ceil4(C[i]) floats); offsets are multiples of 4 */
int hrv_spade_vec_prep_multi_f32(int32_t n, const float* const* gamma_bias, const float* const* beta_bias, const float* const* noise_scale,
                                 const int32_t* C, const int32_t* off_bias, const int32_t* off_noise, float* bias_interleaved_all,
                                 float* noise_scale_padded_all, hrv_stream_t stream);
int hrv_shared_taps_prep_f32(const float* const* w, const float* const* b, int32_t n, int32_t hid, int32_t c, int32_t cp,
                             float* wt, float* bt, hrv_stream_t stream);
int hrv_shared_taps_grad_f32(const float* dw, const float* db, int32_t n, int32_t hid, int32_t c, int32_t cp,
                             float* const* gw, float* const* gb, hrv_stream_t stream);
/* The same power iteration for EVERY spectral-normalised convolution of a network in four launches (27 layers in the
 * SPADE generator, network_generator.py:121-143 via add_spectral_norm; per layer it is eight launches of microseconds).
 * u_keep / v_keep (optional): copies of the (u, v) that produced sigma, for the backward.  wv_scratch: sum of R floats. */
typedef struct {
  const float* w;         /* weight_orig as [R][K] */
  float *u, *v;           /* updated in place when power_iterations > 0 */
  float* sigma;           /* one float per job */
  float *u_keep, *v_keep; /* or NULL */
  int32_t R, K;
} hrv_sn_job_t;
int hrv_spectral_norm_batched_f32(const hrv_sn_job_t* jobs, int32_t n_jobs, int32_t power_iterations, float eps,
                                  float* wv_scratch, hrv_stream_t stream);

/* Scratch the engine would like for this launch (0: none).  Layers with fewer than
 * ~192 output tiles split their K range over up to 32 blocks per tile (partials in
 * the workspace, fixed-order reduction + epilogue in a second kernel: deterministic). */
int64_t hrv_conv2d_workspace_bytes(const hrv_conv2d_t* d);
int hrv_conv2d_nhwc_f32(const hrv_conv2d_t* d, hrv_stream_t stream);
/* bf16 storage / fp32 accumulate flavour of the same engine (v_mfma_f32_32x32x16_bf16): sources,
 * packed weights, residual, the SPADE x tensor and the output are bf16 (uint16_t bit patterns);
 * scale / shift / mean / rstd / noise stay fp32.  Channel counts, strides and offsets are multiples
 * of 8 (one 16-byte gather group).  Same descriptor; w_packed from hrv_conv2d_pack_weight_bf16. */
int64_t hrv_conv2d_packed_elems_bf16(int32_t Cout, int32_t KH, int32_t KW, int32_t nsrc, const int32_t* srcC,
                                     int32_t tile_cfg);
int hrv_conv2d_pack_weight_bf16(const float* w_oihw, int32_t Cout, int32_t KH, int32_t KW, int32_t nsrc,
                                const int32_t* srcC, const int32_t* srcC_real, int32_t tile_cfg, uint16_t* out);
int hrv_conv2d_nhwc_bf16(const hrv_conv2d_t* d, hrv_stream_t stream);
/* Same contract, one thread per output element, raw OIHW weights.  A device
 * side cross-check used by the tests to localise faults; never on the product
 * path. */
int hrv_conv2d_naive_nhwc_f32(const hrv_conv2d_t* d, hrv_stream_t stream);

/* Second half of a KxK stride-1 'same' convolution with a tiny Cout (the
 * 768->2 flow_conv, networks.py:85-92,122,137), run as a 1x1 convolution with
 * KH*KW*Cout "tap channels" on the conv engine (input read once, 16x fewer
 * padded MFMA columns) followed by this gather:
 *   out[p][co] = bias[co] + sum_tap y[p + off(tap)][tap*Cout + co] (+ residual[p][co]) */
int hrv_tapsum_nhwc_f32(const float* y, int32_t N, int32_t H, int32_t W, int32_t KH, int32_t KW, int32_t pad,
                        int32_t Cout, int32_t y_cstride, const float* bias, const float* residual,
                        int32_t res_cstride, float* out, int32_t out_cstride, hrv_stream_t stream);

/* ------------------------------------------------------------------------
 * InstanceNorm2d(affine=False) pieces (network_generator.py:86,427; eps 1e-5,
 * biased variance over H*W per (n,c)).  stats: mean/rstd of x (+ SPADE noise
 * z[n,w,h]*noise_scale[c], :104-110) -- two deterministic stages (shifted
 * partial sums, double-precision fixed-order finalise); `workspace` needs
 * hrv_instnorm_workspace_elems floats.  apply: out = act((x-mean)*rstd).
 * avgpool: F.avg_pool2d(3, stride 2, pad 1, count_include_pad=False) (:301-302).
 * ---------------------------------------------------------------------- */
int64_t hrv_instnorm_workspace_elems(int32_t N, int32_t H, int32_t W, int32_t C);
int hrv_instnorm_stats_nhwc_f32(const float* x, int32_t N, int32_t H, int32_t W, int32_t C, int32_t cstride,
                                int32_t coff, const float* noise_z, const float* noise_scale, float eps,
                                float* workspace, float* mean, float* rstd, hrv_stream_t stream);
/* Two normalisations of the SAME x with different noise terms (norm_0 and norm_s of a learned-shortcut SPADEResBlock,
 * network_generator.py:158-166) in one pass over x; workspace: 2 x hrv_instnorm_workspace_elems floats.  Results are
 * bit-identical to two hrv_instnorm_stats_nhwc_f32 calls. */
int hrv_instnorm_stats2_nhwc_f32(const float* x, int32_t N, int32_t H, int32_t W, int32_t C, int32_t cstride, int32_t coff,
                                 const float* z_a, const float* ns_a, const float* z_b, const float* ns_b, float eps, float* workspace,
                                 float* mean_a, float* rstd_a, float* mean_b, float* rstd_b, hrv_stream_t stream);
/* ... the same over x = cat(nearest_up2(lo), hi) (see hrv_norm_bwd_t: x_up_channels), C = up_channels + channels of hi */
int hrv_instnorm_stats2_up_nhwc_f32(const float* lo, int32_t lo_cstride, int32_t lo_coff, int32_t up_channels, const float* hi,
                                    int32_t hi_cstride, int32_t hi_coff, int32_t N, int32_t H, int32_t W, int32_t C, const float* z_a,
                                    const float* ns_a, const float* z_b, const float* ns_b, float eps, float* workspace, float* mean_a,
                                    float* rstd_a, float* mean_b, float* rstd_b, hrv_stream_t stream);
int hrv_instnorm_stats_nhwc_bf16(const uint16_t* x, int32_t N, int32_t H, int32_t W, int32_t C, int32_t cstride,
                                 int32_t coff, const float* noise_z, const float* noise_scale, float eps,
                                 float* workspace, float* mean, float* rstd, hrv_stream_t stream);
int hrv_instnorm_apply_nhwc_f32(const float* x, int32_t N, int32_t H, int32_t W, int32_t C, int32_t cstride,
                                int32_t coff, const float* mean, const float* rstd, int32_t act, float act_slope,
                                float* out, int32_t out_cstride, int32_t out_coff, hrv_stream_t stream);
int hrv_avgpool3x3s2_nhwc_f32(const float* x, int32_t N, int32_t H, int32_t W, int32_t C, int32_t cstride,
                              int32_t coff, float* out, int32_t out_cstride, int32_t out_coff,
                              hrv_stream_t stream);

/* ------------------------------------------------------------------------
 * Parse-map glue between the two networks (test_generator.py:161-217;
 * train_generator.py:217-275).
 *   mul_channel : fake_segmap[:,3] *= warped_cm (:167-176; binarize=1 is the
 *                 'detach' composition: (cm > 0.5))
 *   gauss_blur  : tgm.image.GaussianBlur((k,k),(s,s)) = depthwise conv with zero
 *                 padding, run as two separable passes; `taps_host` are the k
 *                 normalised 1-D weights (HOST pointer, copied into the launch);
 *                 `tmp` is a scratch tensor of the input's size (:179)
 *   parse_argmax: argmax(dim=1) (first maximum wins) -> int64 labels (nullable)
 *                 + the 13->7 merged one-hot map, NHWC [.,8] (:180-203)
 *   occlusion   : remove_overlap(softmax(gauss), cm) and cloth compositing
 *                 (:19-24,214-216); cm lives in channel cm_ch of an NHWC tensor
 * ---------------------------------------------------------------------- */
int hrv_mul_channel_nhwc_f32(float* x, int32_t x_cstride, int32_t ch, const float* m, int32_t m_cstride,
                             int32_t m_ch, int32_t binarize, int64_t npix, hrv_stream_t stream);
int hrv_gauss_blur_nhwc_f32(const float* in, int32_t N, int32_t H, int32_t W, int32_t C, int32_t cstride,
                            const float* taps_host, int32_t ksize, float* tmp, float* out, hrv_stream_t stream);
int hrv_parse_argmax_nhwc_f32(const float* g, int32_t cstride, int32_t nclass, int64_t npix, int64_t* labels,
                              float* parse7, int32_t parse_cstride, hrv_stream_t stream);
/* F.interpolate(size=(Ho,Wo), mode='bilinear'|'nearest') on contiguous NCHW planes
 * (planes = N*C): the input pre-processing of test_generator.py:144-150. */
int hrv_resize_nchw_f32(const float* in, int32_t planes, int32_t H, int32_t W, int32_t Ho, int32_t Wo,
                        int32_t nearest, float* out, hrv_stream_t stream);
int hrv_occlusion_nhwc_f32(const float* g, int32_t g_cstride, int32_t nclass, float* cloth, int32_t cloth_cstride,
                           float* cm, int32_t cm_cstride, int32_t cm_ch, int64_t npix, hrv_stream_t stream);

/* ------------------------------------------------------------------------
 * Layout converters at the module boundary (the reference's tensors are NCHW).
 * NCHW -> NHWC writes channels [out_coff, out_coff + C) of every pixel and, when the caller asks for it, ``zero_tail``
 * further channels [out_coff + C, out_coff + C + zero_tail) as zeros (the pad channels of a tensor the caller owns
 * whole: the conv engine requires zero pads, and this saves a fill of the whole tensor).  zero_tail == 0 touches nothing
 * outside the slice -- the form to use when ``out`` is one slice of a wider concatenation buffer.
 * ---------------------------------------------------------------------- */
int hrv_nchw_to_nhwc_f32(const float* in, int32_t N, int32_t C, int32_t H, int32_t W, float* out,
                         int32_t out_cstride, int32_t out_coff, int32_t zero_tail, hrv_stream_t stream);
int hrv_nhwc_to_nchw_f32(const float* in, int32_t in_cstride, int32_t in_coff, int32_t N, int32_t C,
                         int32_t H, int32_t W, float* out, hrv_stream_t stream);
/* Space-to-depth by 2 and its inverse over NHWC fp32: out[n][y/2][x/2][((y&1)*2 + (x&1))*C + c] = in[n][y][x][c].  Host side
 * (gen_train.S2DConv): PatchGAN's first convolution -- 4x4, stride 2, pad 2 over 10 channels (network_generator.py
 * NLayerDiscriminator model0) -- runs as a 2x2 stride-1 pad-1 convolution over the 4C-channel tensor. */
int hrv_space_to_depth2_nhwc_f32(const float* in, int32_t N, int32_t H, int32_t W, int32_t C, int32_t in_cstride,
                                 int32_t in_coff, float* out, hrv_stream_t stream);
/* Stride-1 convolutions with ONE output channel (K <= 4): PatchGAN's last layer -- Conv2d(nf, 1, kernel_size=4, stride=1,
 * padding=2) of network_generator.py NLayerDiscriminator and networks.py:389-393 -- forward, data gradient (+ an optional
 * tensor added to dx) and weight / bias gradient as dot-product / outer-product / reduction kernels (the implicit-GEMM engine
 * pads the single column to a 64-column tile).  fp32 FMAs; round_bf16: both operands rounded to bf16 first (the arithmetic
 * of the bf16 matrix-core engine in mixed-precision training).  y is the forward OUTPUT and the backward's dY:
 * [N][H+2*pad-K+1][W+2*pad-K+1][y_cstride], channel y_coff. */
typedef struct {
  const float* x; int32_t N, H, W, C, x_cstride, x_coff;
  const float* w_oihw;             /* [1][C][K][K] */
  const float* sigma; float wscale; /* weights are multiplied by wscale / sigma[0] (sigma may be null) */
  const float* bias;               /* [1] or null (forward) */
  int32_t K, pad;
  float* y; int32_t y_cstride, y_coff;
  float* dx; int32_t dx_cstride, dx_coff;            /* data gradient output [N][H][W][dx_cstride] */
  const float* add; int32_t add_cstride, add_coff;   /* optional: dx = dgrad + add */
  float* workspace;                /* weight gradient: hrv_conv_cout1_wgrad_slabs() * (C*K*K + 1) floats */
  int32_t round_bf16;
} hrv_conv_cout1_t;
int hrv_conv_cout1_fwd_f32(const hrv_conv_cout1_t* d, hrv_stream_t stream);
int hrv_conv_cout1_dgrad_f32(const hrv_conv_cout1_t* d, hrv_stream_t stream);
int32_t hrv_conv_cout1_wgrad_slabs(int32_t N, int32_t Ho, int32_t Wo);
int hrv_conv_cout1_wgrad_f32(const hrv_conv_cout1_t* d, float* dw, int32_t accumulate, float* dbias, int32_t dbias_accumulate,
                             hrv_stream_t stream);
/* cat((a, b), 1) for a NHWC (channels [a_coff, a_coff+Ca) of a_cstride) and b NCHW [N,Cb,H,W], written NHWC
 * [N,H,W,out_cstride] with zeroed pad channels: the PatchGAN input of train_generator.py:283-284. */
int hrv_concat_nhwc_nchw_f32(const float* a, int32_t Ca, int32_t a_cstride, int32_t a_coff, const float* b, int32_t Cb, int32_t N,
                             int32_t H, int32_t W, float* out, int32_t out_cstride, hrv_stream_t stream);
int hrv_depth_to_space2_nhwc_f32(const float* in, int32_t N, int32_t H, int32_t W, int32_t C, float* out, hrv_stream_t stream);

/* ---- DiffAugment (color, translation, cutout) inside the PatchGAN input assembly (diffaug.hip; diffaug.py) ----
 * The augmenting twins of hrv_concat_nhwc_nchw_f32 and of the hrv_nhwc_to_nchw_f32 slice that extracts d(fake), for the PatchGAN
 * shape only: a parse map NHWC with channel stride 8 and Ca <= 8 real channels, an image NCHW [N,3,H,W], an output (gradient) NHWC
 * with channel stride 12; anything else is an argument error.  fp32 storage.  `policy` is a set of HRV_DIFFAUG_* bits; a transform
 * that is absent takes its identity.  u fp32 [N][8] on the device holds uniforms in [0, 1); row n serves sample n.  Decode, in fp32
 * with truncation toward zero:
 *   color        beta = u0 - 0.5,  s = 2 u1,  k = u2 + 0.5
 *   translation  ty = min((int)(u3 (2 Sy + 1)), 2 Sy) - Sy with Sy = (H + 4) / 8;  tx likewise from u4 and W
 *   cutout       a box of ch = H / 2 by cw = W / 2: oy = min((int)(u5 (H + 1 - ch % 2)), H - ch % 2), rows oy - ch / 2 <= y <
 *                oy - ch / 2 + ch; columns likewise from u6 and W; clipped to the image
 * Forward, destination (y, x) of sample n: the source is (y + ty, x + tx); V = the source lies inside the image and (y, x) lies
 * outside the box.  V: out[0:Ca] = parse[source], out[Ca + c] = k s x_c + k (1 - s) m + (1 - k) M + beta with x_c the image at the
 * source, m the mean of its three channels there, M = mean[n] the mean of the whole un-translated image.  Not V: all twelve floats
 * are 0 -- a select: the source is not read, and the address of a source outside the image is never formed.  Pad channels are 0.
 * Backward, with G = V ? g : 0 over destinations: d_img[c, y', x'] = k s G_c(dst) + (k (1 - s) / 3) sum_c' G_c'(dst) +
 * ((1 - k) / (3 H W)) gsum[n], dst = (y' - ty, x' - tx); the first two terms are 0 where dst lies outside the image.  Color is
 * evaluated in fp64 from the fp32 decode and rounded once; without HRV_DIFFAUG_COLOR both directions copy bits. */
enum { HRV_DIFFAUG_COLOR = 1, HRV_DIFFAUG_TRANSLATION = 2, HRV_DIFFAUG_CUTOUT = 4 };
#define HRV_DIFFAUG_SLOTS 128 /* partial sums per sample of the two reductions below */
/* mean[j] = (float)(sum of sample j in fp64 / (3 H W)) for the N samples of `fake`, then (real != NULL) the N samples of `real`: one
 * partial pass over both halves and a one-block-per-sample finalisation, fixed order (bit-identical between runs).  part: fp64
 * [2N][HRV_DIFFAUG_SLOTS] scratch.  A sample's base needs 4-byte alignment only. */
int hrv_diffaug_mean_f32(const float* fake, const float* real, int32_t N, int32_t H, int32_t W, double* part, float* mean,
                         hrv_stream_t stream);
/* a, out 16-byte aligned; mean fp32 [N] (may be NULL without HRV_DIFFAUG_COLOR) */
int hrv_diffaug_concat_f32(const float* a, int32_t Ca, int32_t a_cstride, const float* b, const float* u, const float* mean,
                           int32_t policy, int32_t N, int32_t H, int32_t W, float* out, int32_t out_cstride, hrv_stream_t stream);
/* sum[n] (fp64) = sum of G over the destinations and channels [Ca, Ca + 3) of g NHWC [N,H,W,12]; part: fp64 [N][HRV_DIFFAUG_SLOTS] */
int hrv_diffaug_gsum_f32(const float* g, int32_t g_cstride, int32_t Ca, const float* u, int32_t policy, int32_t N, int32_t H,
                         int32_t W, double* part, double* sum, hrv_stream_t stream);
/* d_img fp32 NCHW [N,3,H,W], every element written; gsum fp64 [N] (may be NULL without HRV_DIFFAUG_COLOR) */
int hrv_diffaug_bwd_f32(const float* g, int32_t g_cstride, int32_t Ca, const float* u, const double* gsum, int32_t policy, int32_t N,
                        int32_t H, int32_t W, float* d_img, hrv_stream_t stream);
/* The gated twins (adaptive discriminator augmentation, Karras et al. 2020): the signature of the ungated sibling plus
 *   ug  device fp32 [N][4], uniforms in [0, 1): column 0 gates color, 1 translation, 2 cutout; column 3 is spare and never read
 *   p   device, ONE fp64 (8-byte aligned), read by the kernel: no host copy, so a controller on the device may move it
 * Sample n runs everything above under its effective policy
 *   policy & (((double)ug[n][0] < p[0] ? COLOR : 0) | ((double)ug[n][1] < p[0] ? TRANSLATION : 0) | ((double)ug[n][2] < p[0] ? CUTOUT : 0))
 * with a strict comparison in fp64: p == 0 applies nothing, p == 1 everything, ug == p does not apply.  A sample whose effective
 * policy is 0 copies bits in both directions.  The gate is decoded once per block with u's row (the block is the sample).  Color
 * is gated as one group.  hrv_diffaug_mean_f32 serves both forms; the mean of a sample whose color is gated off is not read. */
int hrv_diffaug_concat_gated_f32(const float* a, int32_t Ca, int32_t a_cstride, const float* b, const float* u, const float* mean,
                                 int32_t policy, int32_t N, int32_t H, int32_t W, float* out, int32_t out_cstride, const float* ug,
                                 const double* p, hrv_stream_t stream);
int hrv_diffaug_gsum_gated_f32(const float* g, int32_t g_cstride, int32_t Ca, const float* u, int32_t policy, int32_t N, int32_t H,
                               int32_t W, double* part, double* sum, const float* ug, const double* p, hrv_stream_t stream);
int hrv_diffaug_bwd_gated_f32(const float* g, int32_t g_cstride, int32_t Ca, const float* u, const double* gsum, int32_t policy,
                              int32_t N, int32_t H, int32_t W, float* d_img, const float* ug, const double* p, hrv_stream_t stream);

/* The controller of p: one launch of one block after hrv_dhead_forward_f32 of the discriminator step; dhead_record is that head's
 * record (below), state HRV_ADA_WORDS doubles, zeroed once (P may be preset), every word fp64.  The gates read &state[HRV_ADA_P].
 * All arithmetic is IEEE fp64 in exactly this order:
 *   1. STEPS += 1                                            (calls so far, poisoned ones included)
 *   2. record[HRV_DHEAD_NONFINITE] != 0: return              (a poisoned step is neither accumulated nor counted in the window)
 *   3. sum = 0; for k = 0 .. num_d - 1 ascending: sum += record[HRV_DHEAD_STATE + HRV_DHEAD_SCALE_WORDS * k + HRV_DHEAD_RT];
 *      r = sum / (double)num_d
 *   4. RT_LAST = r; ACC += r; SEEN += 1
 *   5. SEEN == interval: m = ACC / (double)interval; RT_WINDOW = m; s = (m > target) - (m < target);
 *      P = min(max(P + s * step, 0), p_max); ACC = SEEN = 0; UPDATES += 1
 * (s * step is exact, so a fused multiply-add gives the same P.)  target in [-1, 1], step and p_max in [0, 1], interval >= 1.
 * StyleGAN2-ADA's rule is step = images_per_step * interval / (kimg * 1000) with images_per_step the global batch. */
#define HRV_ADA_WORDS 8
#define HRV_ADA_P 0         /* the probability the gates read */
#define HRV_ADA_ACC 1       /* sum of r over the open window */
#define HRV_ADA_SEEN 2      /* steps in the open window */
#define HRV_ADA_UPDATES 3   /* adjustments made so far */
#define HRV_ADA_RT_WINDOW 4 /* mean r of the last closed window */
#define HRV_ADA_STEPS 5     /* calls so far */
#define HRV_ADA_RT_LAST 6   /* r of the last accumulated step */
int hrv_ada_update_f64(const double* dhead_record, int32_t num_d, double target, double step, int32_t interval, double p_max,
                       double* state, hrv_stream_t stream);

/* Fused loss head of the PatchGAN's discriminator step: hinge terms, logit statistics, LeCam anchors and regulariser (Tseng et al.,
 * CVPR 2021) and the gradients of all logits, decided ON THE DEVICE (no host read, capturable).  Per scale k < num_d (at most
 * HRV_DHEAD_MAX_SCALES): x_fake[k] / x_real[k] point at n[k] dense fp32 logits each (any 4-byte-aligned pointer, any n >= 1; nothing
 * outside is read).  The three pointer / count arrays are HOST arrays, read during the call.
 *
 * hrv_dhead_forward_f32.  stage: bit 0 launches the reduce pass (logits -> part), bit 1 a finalize block that turns part into the sums
 * of the record, bit 2 a finalize block that turns the sums into everything else (bits 1 and 2 together: one launch); 7 = the whole
 * forward in two launches.  part: HRV_DHEAD_PART_WORDS doubles of scratch.  record:
 * HRV_DHEAD_WORDS doubles, zeroed once before the first step, every word fp64:
 *   [HRV_DHEAD_COUNT]      applied anchor updates so far (a poisoned step is not applied)
 *   [HRV_DHEAD_NONFINITE]  this step's count of non-finite logits, all scales
 *   [HRV_DHEAD_LAMBDA]     this step's lambda_eff: weight when COUNT, as it stood BEFORE this step, is >= start, else 0
 *   [HRV_DHEAD_REG]        this step's R, averaged over the scales, before the weight (form relu with lambda_eff == 0: not computed, 0)
 *   [HRV_DHEAD_STEPS]      steps seen, poisoned ones included
 *   [HRV_DHEAD_STATE + HRV_DHEAD_SCALE_WORDS * k + ...]   per scale:
 *     ANCHOR_REAL, ANCHOR_FAKE   a <- d * a + (1 - d) * mean, d = decay, or 0 while COUNT == 0; updated BEFORE they are used
 *     RT_AVG                     the same average of RT
 *     RT, MEAN_REAL, MEAN_FAKE   this step's sum sign(x_real) / n (sign(0) = 0), sum x_real / n, sum x_fake / n
 *     REG_K                      this step's R of the scale
 *   [HRV_DHEAD_SUMS + HRV_DHEAD_SCALE_WORDS * k + ...]    per scale, this step's raw sums in a fixed order:
 *     SUM_REAL, SUM_FAKE, SIGN_REAL, HINGE_REAL (sum max(1 - x_r, 0)), HINGE_FAKE (sum max(1 + x_f, 0)), SUMSQ_REAL, SUMSQ_FAKE,
 *     NONFINITE_K
 * R = mean((x_r - a_F)^2) + mean((x_f - a_R)^2) (HRV_DHEAD_FORM_PAPER) or mean(relu(x_r - a_F)^2) + mean(relu(a_R - x_f)^2)
 * (HRV_DHEAD_FORM_RELU, the published code).  losses[0..2] = D_Fake, D_Real (hinge means averaged over the scales) and
 * D_LeCam = lambda_eff * R, each the fp64 value rounded once.  A poisoned step (NONFINITE != 0) leaves the anchors, RT_AVG and COUNT
 * alone, reports the hinge means as the sums give them and D_LeCam = NaN.
 * n_mult multiplies every n in the means: a data-parallel caller all-reduces record[HRV_DHEAD_SUMS ...] between a stage-2 and a
 * stage-4 call with n_mult = world.  (The relu form's second pass is over the
 * caller's own logits.)  The slot count, the element -> slot rule and every summation order are fixed and no atomics are used: the
 * same logits give the same bits in every run and on every card.
 *
 * hrv_dhead_backward_f32: one launch.  d_fake[k][i] / d_real[k][i] = (+-1 or 0) * (float)(1 / n) * (g / num_d), g = g_fake[0] /
 * g_real[0], in fp32 and in that order, plus -- when lambda_eff != 0 -- (g_lecam[0] / num_d) * lambda_eff * dR/dx in fp64, the sum
 * rounded once.  record is what the forward call of the same step left; the anchors are constants of the gradient. */
#define HRV_DHEAD_MAX_SCALES 4
#define HRV_DHEAD_SLOTS 64
#define HRV_DHEAD_PART_WORDS (2 * HRV_DHEAD_MAX_SCALES * HRV_DHEAD_SLOTS * 5)
#define HRV_DHEAD_FORM_PAPER 0
#define HRV_DHEAD_FORM_RELU 1
#define HRV_DHEAD_COUNT 0
#define HRV_DHEAD_NONFINITE 1
#define HRV_DHEAD_LAMBDA 2
#define HRV_DHEAD_REG 3
#define HRV_DHEAD_STEPS 4
#define HRV_DHEAD_STATE 8
#define HRV_DHEAD_SUMS 40
#define HRV_DHEAD_SCALE_WORDS 8
#define HRV_DHEAD_WORDS 72
#define HRV_DHEAD_ANCHOR_REAL 0
#define HRV_DHEAD_ANCHOR_FAKE 1
#define HRV_DHEAD_RT_AVG 2
#define HRV_DHEAD_RT 3
#define HRV_DHEAD_MEAN_REAL 4
#define HRV_DHEAD_MEAN_FAKE 5
#define HRV_DHEAD_REG_K 6
#define HRV_DHEAD_SUM_REAL 0
#define HRV_DHEAD_SUM_FAKE 1
#define HRV_DHEAD_SIGN_REAL 2
#define HRV_DHEAD_HINGE_REAL 3
#define HRV_DHEAD_HINGE_FAKE 4
#define HRV_DHEAD_SUMSQ_REAL 5
#define HRV_DHEAD_SUMSQ_FAKE 6
#define HRV_DHEAD_NONFINITE_K 7
int hrv_dhead_forward_f32(int32_t num_d, const float* const* x_fake, const float* const* x_real, const int64_t* n, int32_t form,
                          double weight, double decay, int32_t start, int32_t n_mult, int32_t stage, double* part, double* record,
                          float* losses, hrv_stream_t stream);
int hrv_dhead_backward_f32(int32_t num_d, const float* const* x_fake, const float* const* x_real, const int64_t* n, int32_t form,
                           const double* record, const float* g_fake, const float* g_real, const float* g_lecam,
                           float* const* d_fake, float* const* d_real, hrv_stream_t stream);

/* fp32 NCHW (module boundary) <-> bf16 NHWC (inside the bf16 generator path) */
int hrv_nchw_f32_to_nhwc_bf16(const float* in, int32_t N, int32_t C, int32_t H, int32_t W, uint16_t* out,
                              int32_t out_cstride, int32_t out_coff, int32_t zero_tail, hrv_stream_t stream);
int hrv_nhwc_bf16_to_nchw_f32(const uint16_t* in, int32_t in_cstride, int32_t in_coff, int32_t N, int32_t C,
                              int32_t H, int32_t W, float* out, hrv_stream_t stream);

/* ------------------------------------------------------------------------
 * Bilinear resize, align_corners=False (F.interpolate / nn.Upsample bilinear:
 * networks.py:130-133,150,181; test_generator.py:144-150,179,207), NHWC, with
 * an optional fused addend: out = resize(in) + addend   (networks.py:130-131).
 * rh, rw are the source-index ratios: 1/scale_factor, or in/out for size=.
 * ---------------------------------------------------------------------- */
int hrv_resize_bilinear_nhwc_f32(const float* in, int32_t N, int32_t H, int32_t W, int32_t C,
                                 int32_t in_cstride, int32_t in_coff, int32_t Ho, int32_t Wo, float rh,
                                 float rw, const float* addend, int32_t add_cstride, int32_t add_coff,
                                 float* out, int32_t out_cstride, int32_t out_coff, hrv_stream_t stream);

/* ------------------------------------------------------------------------
 * Appearance-flow warp: the fused form of
 *     flow  = F.interpolate(flow_prev, bilinear)            networks.py:133,150
 *     fnorm = flow / (norm_x, norm_y)                        networks.py:134,151
 *     grid  = make_grid(N, Ho, Wo) (= linspace(-1,1))        networks.py:161-168
 *     out   = F.grid_sample(src, fnorm + grid, 'bilinear',
 *                           padding_mode='border',
 *                           align_corners=False)             networks.py:135,152
 * (also test_generator.py:206-213 with size= resize and the hard-coded norms).
 * flow_prev is the reference's own [N,fh,fw,2] (x,y) layout.  flow_up
 * (optional) receives the un-normalised upsampled flow [N,Ho,Wo,2].
 * ---------------------------------------------------------------------- */
typedef struct hrv_flow_warp {
  const float* src;
  int32_t N, H, W, C; /* sampled tensor extent (C multiple of 4)             */
  int32_t src_cstride, src_coff;
  const float* flow;
  int32_t fh, fw;
  int32_t Ho, Wo;
  float rh, rw;
  float norm_x, norm_y;
  float* out;
  int32_t out_cstride, out_coff;
  float* flow_up; /* or NULL */
} hrv_flow_warp_t;
int hrv_flow_warp_nhwc_f32(const hrv_flow_warp_t* d, hrv_stream_t stream);

/* Tap expansion of a narrow NHWC tensor (im2col in 16-byte groups): out[n,h,w, t*G + g] = group g of the
 * source pixel under tap t of a stride-1 'same' KHxKW window (zero outside the image); the source may be
 * 2^down_shift larger (nearest down-sampling, F.interpolate(segmap, 'nearest'), network_generator.py:112).
 * With it the 7-channel conv_shared 3x3 of every SPADENorm (network_generator.py:97,113) runs as a 1x1
 * convolution over KH*KW*G*16 dense bytes per pixel.  Strides / offsets in 16-byte units; any element type. */
int hrv_tap_expand_nhwc(const void* src, int32_t N, int32_t H, int32_t W, int32_t group16_per_pixel,
                        int32_t src_stride16, int32_t src_off16, int32_t down_shift, int32_t KH, int32_t KW,
                        int32_t pad, void* out, hrv_stream_t stream);

/* ------------------------------------------------------------------------
 * Training of the condition generator (train_condition.py:113-286, tocg.train()).
 *
 * BatchNorm2d with batch statistics (networks.py:171-198 under train_condition.py:116):
 *   bn_finalize : folds the per-sample (mean, rstd) of hrv_instnorm_stats_nhwc_f32
 *                 (computed with eps_in) into batch mean / rstd (biased variance over
 *                 N*H*W, eps), the affine y = scale*x + shift (scale = gamma*rstd) and
 *                 nn.BatchNorm2d's running-statistics update (momentum, unbiased variance);
 *                 running_* may be NULL.  Writes entries c < C only.
 *   affine_act  : out = act(x*scale[c] + shift[c] (+ residual))   (BN apply + ReLU + skip)
 *   bn_bwd      : dx (+)= scale*(dy - mean(dy) - xhat*mean(dy*xhat)), dgamma (+)= sum dy*xhat,
 *                 dbeta (+)= sum dy; x is the convolution output the statistics were taken
 *                 of.  mean / rstd / scale hold ceil4(C) floats (zero in the pad channels);
 *                 workspace: hrv_bn_bwd_workspace_elems(C) floats.  Deterministic.
 * ---------------------------------------------------------------------- */
int hrv_bn_finalize_f32(const float* mean_nc, const float* rstd_nc, int32_t N, int32_t C, int32_t nc_stride,
                        float eps_in, int64_t HW, const float* gamma, const float* beta, float eps, float momentum,
                        float* running_mean, float* running_var, float* mean, float* rstd, float* scale, float* shift,
                        hrv_stream_t stream);
int hrv_affine_act_nhwc_f32(const float* x, int32_t x_cstride, int32_t x_coff, int32_t C, int64_t npix,
                            const float* scale, const float* shift, const float* residual, int32_t res_cstride,
                            int32_t res_coff, int32_t act, float act_slope, float* out, int32_t out_cstride,
                            int32_t out_coff, hrv_stream_t stream);
int64_t hrv_bn_bwd_workspace_elems(int32_t C);
int hrv_bn_bwd_nhwc_f32(const float* dy, int32_t dy_cstride, int32_t dy_coff, const float* x, int32_t x_cstride,
                        int32_t x_coff, int32_t C, int64_t npix, const float* mean, const float* rstd, const float* scale,
                        float* workspace, float* dx, int32_t dx_cstride, int32_t dx_coff, int32_t dx_accumulate,
                        float* dgamma, float* dbeta, int32_t dgb_accumulate, hrv_stream_t stream);
/* Adjoint of hrv_resize_bilinear_nhwc_f32 (F.interpolate / nn.Upsample backward,
 * networks.py:130-133,150,181; train_condition.py:242): dx[N,H,W,C] (+)= R^T dy[N,Ho,Wo,C],
 * gather form (deterministic).  Any C (an NCHW tensor is the C = 1 case with N*C planes). */
int hrv_resize_bilinear_bwd_nhwc_f32(const float* dy, int32_t N, int32_t Ho, int32_t Wo, int32_t C, int32_t dy_cstride,
                                     int32_t dy_coff, float rh, float rw, float* dx, int32_t H, int32_t W,
                                     int32_t dx_cstride, int32_t dx_coff, int32_t accumulate, hrv_stream_t stream);
/* F.interpolate(mode='nearest') over planes [planes][H][W] -> [planes][Ho][Wo] (an NCHW tensor: planes = N*C) and its adjoint
 * (gather form, deterministic): the inter-flow loss of train_condition.py:242 under --upsample nearest.  torch's legacy nearest:
 * src = min(floorf(dst * (float)in / out), in - 1). */
int hrv_resize_nearest_nchw_f32(const float* in, int32_t planes, int32_t H, int32_t W, int32_t Ho, int32_t Wo, float* out,
                                hrv_stream_t stream);
int hrv_resize_nearest_nchw_bwd_f32(const float* dout, int32_t planes, int32_t Ho, int32_t Wo, int32_t H, int32_t W, float* dx,
                                    hrv_stream_t stream);
/* The same nearest selection over NHWC activations (any C, channel slices), out = nearest(in) (+ addend), and its adjoint
 * dx (+)= N^T dout: ConditionGenerator.forward(upsample='nearest') -- networks.py:130-131 (T = up(T) + conv1x1(E)), :133 / :150 (the
 * flow upsampled by 2 in front of the warp; the warp kernel then reads it at ratio 1). */
int hrv_resize_nearest_nhwc_f32(const float* in, int32_t N, int32_t H, int32_t W, int32_t C, int32_t in_cstride, int32_t in_coff,
                                int32_t Ho, int32_t Wo, const float* addend, int32_t add_cstride, int32_t add_coff, float* out,
                                int32_t out_cstride, int32_t out_coff, hrv_stream_t stream);
int hrv_resize_nearest_bwd_nhwc_f32(const float* dout, int32_t N, int32_t Ho, int32_t Wo, int32_t C, int32_t d_cstride, int32_t d_coff,
                                    float* dx, int32_t H, int32_t W, int32_t dx_cstride, int32_t dx_coff, int32_t accumulate,
                                    hrv_stream_t stream);
/* Adjoint of hrv_flow_warp_nhwc_f32 (F.grid_sample backward, networks.py:135,152): given the
 * saved un-normalised flow at the output resolution (flow_up) and dout [N,Ho,Wo,C]:
 *   dsrc  [N,H,W,C]   += scatter of the four bilinear taps (fp32 atomics; zero-init or an
 *                        existing accumulator; may be NULL)
 *   dflow [N,Ho,Wo,2] (+)= d/d flow_up (coordinate gradient x W/2 (H/2) / norm; zero where the
 *                        sample position was clamped to the border, as torch does; may be NULL). */
typedef struct hrv_flow_warp_bwd {
  const float* src;
  int32_t N, H, W, C;
  int32_t src_cstride, src_coff;
  const float* flow_up;
  int32_t Ho, Wo;
  float norm_x, norm_y;
  const float* dout;
  int32_t dout_cstride, dout_coff;
  float* dsrc;
  int32_t dsrc_cstride, dsrc_coff;
  float* dflow;
  int32_t dflow_accumulate;
  int32_t _pad;
} hrv_flow_warp_bwd_t;
int hrv_flow_warp_bwd_nhwc_f32(const hrv_flow_warp_bwd_t* d, hrv_stream_t stream);
/* F.grid_sample(input NCHW, grid [N,Ho,Wo,2], 'bilinear', padding_mode='border',
 * align_corners=False) with an explicit grid, and its backward (train_condition.py:243-245;
 * train_generator.py:237-238).  din (+= atomics, zero-init) and dgrid may each be NULL. */
int hrv_grid_sample_nchw_f32(const float* in, int32_t N, int32_t C, int32_t H, int32_t W, const float* grid, int32_t Ho,
                             int32_t Wo, float* out, hrv_stream_t stream);
int hrv_grid_sample_nchw_bwd_f32(const float* in, int32_t N, int32_t C, int32_t H, int32_t W, const float* grid,
                                 int32_t Ho, int32_t Wo, const float* dout, float* din, float* dgrid,
                                 hrv_stream_t stream);
/* torch.softmax(x, 1) on NCHW (train_condition.py:175,246,260) and its backward
 * dx = y*(dy - sum_c dy*y); C <= 64. */
int hrv_softmax_nchw_f32(const float* x, int32_t N, int32_t C, int64_t HW, float* y, hrv_stream_t stream);
int hrv_softmax_nchw_bwd_f32(const float* y, const float* dy, int32_t N, int32_t C, int64_t HW, float* dx,
                             hrv_stream_t stream);
/* utils.cross_entropy2d (utils.py:29-42): mean over the valid pixels of logsumexp(x) - x[target]
 * (targets outside [0,C) are ignored like ignore_index=250); loss_out[0] = loss, loss_out[1] =
 * valid-pixel count; grad (optional, NCHW) = gscale*(softmax - onehot) -- the caller folds
 * 1/count into gscale.  workspace: 1024 floats. */
int hrv_cross_entropy_nchw_f32(const float* x, const int64_t* target, int32_t N, int32_t C, int64_t HW, float gscale,
                               float* grad, float* workspace, float* loss_out, hrv_stream_t stream);
/* Adjoint of hrv_tapsum_nhwc_f32 (the 768->2 flow_conv, networks.py:85-92, run as a
 * taps-as-channels 1x1 convolution): dy[q][tap*Cout+co] = dout[q - off(tap)][co]; dy has
 * ceil4(KH*KW*Cout) channels (padding zeroed). */
int hrv_tapsum_bwd_nhwc_f32(const float* dout, int32_t N, int32_t H, int32_t W, int32_t KH, int32_t KW, int32_t pad,
                            int32_t Cout, int32_t dout_cstride, float* dy, int32_t dy_cstride, hrv_stream_t stream);
/* out = x * m elementwise (dense buffers, n % 4 == 0): nn.Dropout(0.5) of the tocg discriminator with the keep
 * mask pre-scaled by 1/(1-p) (networks.py:363-368), forward and backward. */
int hrv_mul_f32(const float* x, const float* m, int64_t n, float* out, hrv_stream_t stream);
/* Flow total variation (train_condition.py:190-199) of one [N,H,W,2] flow:
 * loss = mean|f[:,1:]-f[:,:-1]| + mean|f[:,:,1:]-f[:,:,:-1]|, grad = d loss / d f (optional).
 * workspace: 1024 floats. */
int hrv_tv_loss_f32(const float* flow, int32_t N, int32_t H, int32_t W, float* grad, float* workspace, float* loss_out,
                    hrv_stream_t stream);

/* SPADENorm's conv_gamma || conv_beta (network_generator.py:117-121: two 3x3 convolutions 128 -> C over
 * actv = ReLU(conv_shared(seg))) fused with `normalized * (1 + gamma) + beta` (+ LeakyReLU, :170-171), and the data
 * gradient of that pair, d(actv) = conv^T([dgamma | dbeta]) * relu'(actv), on a dedicated kernel (csrc/spade_gb.hip):
 * one persistent 8-wave block per CU owns a 16x16-pixel tile and ALL of the layer's columns (no padded columns, the
 * halo patch loaded once), weights streamed in MFMA-fragment order through a 3-stage LDS ring.
 *   mode 0 (forward):  src = actv, bf16 NHWC [.,hid]; columns = (gamma | beta) of the C norm channels;
 *                      out = act((x + z*noise_scale - mean) * rstd * (1 + gamma + bias_gamma) + beta + bias_beta);
 *                      g1p (optional) receives (1 + gamma), dense [pixels][stat_stride], fp32 or bf16.
 *   mode 1 (data gradient): src = [dgamma (Cp) | dbeta (Cp)], bf16 NHWC; out[.., hid] = conv^T * (mask > 0 ? 1 :
 *                      act_slope), mask = actv (bf16) or NULL.
 * Shapes served: hid == 128, C % 32 in {0, 16} (32, 64, 80, 128, 144, 272, 528, ...; not 48: one pair + tail),
 * at least 256 tiles (hrv_spade_gb_supported); everything else keeps hrv_conv2d_nhwc_bf16's tiles. */
typedef struct hrv_spade_gb {
  int32_t mode, N, H, W;
  const void* src; int32_t src_cstride, src_coff;
  const void* w_packed;        /* hrv_spade_gb_pack_dev(mode, ...)                                   */
  int32_t C, Cp, hid;          /* norm channels, their padded count (layout of [dgamma|dbeta]), 128  */
  int32_t x_f32;               /* forward: x is fp32 (else bf16)                                     */
  const void* x; int32_t x_cstride, x_coff;
  int32_t stat_stride;         /* floats per image in mean / rstd, channels per pixel in g1p        */
  int32_t g1p_bf16;
  const float* mean; const float* rstd; const float* noise_z; const float* noise_scale;
  const float* bias_gamma; const float* bias_beta;
  void* g1p;
  int32_t act; float act_slope;
  void* out; int32_t out_cstride, out_coff, out_f32, _pad;
  const void* mask; int32_t mask_cstride, mask_coff;
} hrv_spade_gb_t;
int64_t hrv_spade_gb_packed_bytes(int32_t mode, int32_t C, int32_t Cp, int32_t hid);   /* -1: shape not served */
int hrv_spade_gb_supported(int32_t mode, int32_t C, int32_t Cp, int32_t hid, int32_t N, int32_t H, int32_t W);
/* fp32 conv_gamma.weight / conv_beta.weight [C][hid][3][3] (device) -> the bf16 fragment-order stream of `mode` */
int hrv_spade_gb_pack_dev(int32_t mode, const float* w_gamma, const float* w_beta, int32_t C, int32_t Cp, int32_t hid,
                          void* out, hrv_stream_t stream);
int hrv_spade_gb_bf16(const hrv_spade_gb_t* d, hrv_stream_t stream);

/* SPADENorm forward fused end to end (spade_fused.hip; network_generator.py:93-121): replaces, for one norm,
 *     actv  = F.relu(conv_shared(F.interpolate(segmap, size, 'nearest')))            (:115-116)
 *     out   = act(param_free_norm(x + noise) * (1 + conv_gamma(actv)) + conv_beta(actv))   (:104-110, :117-121)
 * `actv` is computed inside the kernel from the label patch (two blocks per CU; it never travels through HBM unless the
 * caller asks for it).
 *   seg      bf16 NHWC [N, H << seg_shift, W << seg_shift, 8] (label_nc <= 8 real channels, the rest zero): the level's
 *            nearest-downsampled label map is read in place (pixel (y << seg_shift, x << seg_shift));
 *   w_packed hrv_spade_fused_pack_dev(conv_shared.weight / .bias, conv_gamma.weight, conv_beta.weight);
 *   x        fp32 (x_f32 = 1) or bf16 NHWC slice; mean / rstd [N][C]; noise_z [N][W][H] + noise_scale [C] or both NULL;
 *   out      bf16 NHWC slice; g1p (optional) <- 1 + gamma, bf16 dense [N,H,W,C];
 *   actv     (optional) <- ReLU(conv_shared(seg)), bf16 NHWC slice of 128 channels (the training forward keeps it for
 *            the backward: ReLU mask of the data gradient, operand of the gamma|beta weight gradient).
 * Shapes served: hid == 128, C % 32 in {0, 16}, C >= 32, at least two tiles per CU (hrv_spade_fused_supported). */
typedef struct hrv_spade_fused {
  int32_t N, H, W, C;
  const void* seg; int32_t seg_H, seg_W, seg_shift, x_f32;
  const void* w_packed;
  const void* x; int32_t x_cstride, x_coff;
  const float* mean; const float* rstd; const float* noise_z; const float* noise_scale;
  const float* bias_gamma; const float* bias_beta;
  void* g1p;
  int32_t act; float act_slope;
  void* out; int32_t out_cstride, out_coff;
  void* actv; int32_t actv_cstride, actv_coff;
  /* x = cat(nearest_up2(lo), hi), never materialised (x_up_channels > 0, a multiple of 16; x fp32): channels [0, x_up_channels) are read
   * from `x` = lo [N][H/2][W/2][x_cstride] at (y >> 1, x >> 1), the rest from `x2` = hi [N][H][W][x2_cstride] (see hrv_norm_bwd_t) */
  int32_t x_up_channels;
  const void* x2; int32_t x2_cstride, x2_coff;
  /* optional tile plan (hrv_spade_tiles_bf16 of the same label map, shift and extent; NULL: every tile does the matrix work):
   * spade_fused_kernel works through the plan's heavy tiles, spade_uniform_kernel (same call, same stream, right behind it) gives
   * the light ones -- one one-hot label over the whole 20x20 patch, gamma|beta a constant -- the epilogue alone, bit-identical.
   * gb_table: fp32 [8][2][C] scratch of this launch (the representatives' gamma|beta).  tiles_phase: 0 both kernels, 1 / 2 only
   * the heavy / the light part (two calls, 1 then 2, are one call with 0: a profiler times the kernels apart). */
  const int32_t* tiles; float* gb_table; int32_t tiles_phase;
} hrv_spade_fused_t;
int64_t hrv_spade_fused_packed_bytes(int32_t C);   /* -1: norm width not served */
int hrv_spade_fused_supported(int32_t C, int32_t hid, int32_t label_nc, int32_t N, int32_t H, int32_t W);
/* conv_shared.weight [128][label_nc][3][3] + bias [128], conv_gamma.weight / conv_beta.weight [C][128][3][3] (fp32, device)
 * -> the bf16 fragment-order stream the kernel's LDS ring consumes */
int hrv_spade_fused_pack_dev(const float* w_shared, const float* b_shared, int32_t label_nc, const float* w_gamma,
                             const float* w_beta, int32_t C, void* out, hrv_stream_t stream);
int hrv_spade_fused_bf16(const hrv_spade_fused_t* d, hrv_stream_t stream);
/* The tile plan of a label map at one level (csrc/spade_tiles.h has the layout: int32 counts [0] heavy, [1] light, [2..9] the
 * representative tile of each class or -1, from word 16 the heavy list, then the light list, patch_tiles(N, H, W) words each).
 * A 16x16-pixel tile is LIGHT with class k when its 20x20 patch of sampled label pixels (y << seg_shift, x << seg_shift) lies wholly
 * inside the H x W level image, all 400 16-byte vectors are bitwise equal and that vector is channel k = bf16 1.0, every other
 * channel 0; every other tile is heavy, and so is the lowest light tile of each class (its representative).  Lists ascend. */
int64_t hrv_spade_tiles_plan_bytes(int32_t N, int32_t H, int32_t W);   /* -1: extent not served */
int hrv_spade_tiles_bf16(const void* seg, int32_t seg_H, int32_t seg_W, int32_t seg_shift, int32_t N, int32_t H, int32_t W,
                         void* plan, hrv_stream_t stream);

/* 3x3 stride-1 'same' convolution over ONE bf16-stored NHWC source, any Cin / Cout (the source keeps its channels padded to 8 with
 * zeros, `out` / `mask` / `residual` theirs padded to 16 bytes: the pad lanes of `out` receive zeros), two blocks per CU
 * (conv_p2.hip): nn.Conv2d forward (VGG19 of the perceptual loss, networks.py:201-233) and data gradients -- of such a
 * convolution (mode 1) or of the SPADE (conv_gamma, conv_beta) pair over [dgamma | dbeta] (mode 2, network_generator.py:117-118).
 *   out = act(conv + bias[c] [+ residual]) [* (mask > 0 ? 1 : mask_slope)] [+ residual, if res_after_mask], bf16 or fp32 NHWC slice.
 * `Cin` = K (channels of `src`), `Cout` = columns, whatever the mode; w_packed from hrv_conv_p2_pack_dev of the same mode:
 *   mode 0: w = the layer's OIHW weight [Cout][Cin][3][3];
 *   mode 1: w = the FORWARD layer's OIHW weight [Cin][Cout][3][3] (its output channels are this call's K), taps flipped;
 *   mode 2: (w, w2) = [Cin / 2][Cout][3][3] each, K = [w rows | w2 rows], taps flipped.
 * `sigma` (optional device scalar) and `wscale`: packed weight = w * wscale / sigma[0].
 * hrv_conv_p2_supported: shape served and at least 1.5 tiles per CU (HRV_CONV_P2_MIN_TILES_X4: the threshold in quarter-tiles). */
typedef struct hrv_conv_p2 {
  int32_t N, H, W, Cin;
  const void* src; int32_t src_cstride, src_coff, Cout;
  const void* w_packed;
  const float* bias;
  int32_t act; float act_slope;
  const void* mask; int32_t mask_cstride, mask_coff; float mask_slope; int32_t out_f32;
  void* out; int32_t out_cstride, out_coff;
  int32_t res_f32;                                           /* residual dtype: 1 fp32, 0 bf16 */
  const void* residual; int32_t res_cstride, res_coff;       /* optional NHWC slice added BEFORE the activation (SPADEResBlock: x_s + dx) */
  int32_t res_after_mask;                                    /* 1: added behind activation and mask instead (a data gradient that meets
                                                              * another gradient of the same tensor: VGG19's tap gradients) */
} hrv_conv_p2_t;
int64_t hrv_conv_p2_packed_bytes(int32_t Cin, int32_t Cout);   /* -1: shape not served */
int hrv_conv_p2_supported(int32_t Cin, int32_t Cout, int32_t N, int32_t H, int32_t W);
int hrv_conv_p2_pack_dev(int32_t mode, const float* w, const float* w2, int32_t Cin, int32_t Cout, const float* sigma, float wscale,
                         void* out, hrv_stream_t stream);
int hrv_conv_p2_bf16(const hrv_conv_p2_t* d, hrv_stream_t stream);

/* PatchGAN's 4x4 stride-2 pad-2 convolution over a bf16-stored NHWC feature map, and its data gradient, as ONE launch family
 * on the two-blocks-per-CU skeleton of hrv_conv_p2_bf16 (conv_s2.hip; NLayerDiscriminator, network_generator.py:263-272:
 * nn.Conv2d(nf_prev, nf, kernel_size=4, stride=2, padding=2) and autograd's gradient w.r.t. its input).
 *   mode 0  forward: src [N][Hs][Ws][K] -> out [N][Ho = Hs/2+1][Wo = Ws/2+1][cols]; w = the layer's OIHW weight [cols][K][4][4].
 *   mode 1  data gradient: src = dY [N][Hs][Ws][K] (K = the forward layer's OUTPUT channels) -> out = dX [N][Ho][Wo][Cph]
 *           (Hs = Ho/2+1), cols = 4 * Cph (the four output phases are column passes); w = the forward OIHW weight [K][Cph][4][4].
 *   mode 2  a 2x2 stride-1 convolution, pad 1 on top / left only: src = a space-to-depth image [N][Hs][Ws][K] -> out
 *           [N][Ho in {Hs, Hs+1}][Wo ...][cols]; w = [cols][K][2][2] (PatchGAN's model0: 10 channels -> 4 x 12 per cell).
 *   out = act(conv + bias[c] [+ residual]) [* (mask > 0 ? 1 : mask_slope)]; residual / mask: slices shaped like `out`.
 * K % 8 == 0 (mode 0: % 32), cols % 64 == 0, Cph % 32 == 0.  w_packed from hrv_conv_s2_pack_dev of the same (mode, K, cols, Cph). */
typedef struct hrv_conv_s2 {
  int32_t mode;
  int32_t N, Hs, Ws, K;
  const void* src; int32_t src_cstride, src_coff;
  int32_t Ho, Wo, cols, Cph;
  const void* w_packed;
  const float* bias;
  int32_t act; float act_slope;
  void* out; int32_t out_cstride, out_coff, out_f32;
  const void* residual; int32_t res_cstride, res_coff, res_f32;
  const void* mask; int32_t mask_cstride, mask_coff; float mask_slope;
} hrv_conv_s2_t;
#define HRV_S2_SPLIT3 4   /* or-ed into hrv_conv_s2_pack_dev's mode (0 / 2): K = 3 K0 over a source laid out [hi | lo | hi]
                           * (hrv_split3_nhwc_bf16), w has K0 input channels and is packed as [hi(w) | hi(w) | w - hi(w)]: the
                           * convolution sums hi*hi + lo*hi + hi*lo -- fp32 operands to ~16 mantissa bits on the bf16 matrix cores
                           * (the half-resolution PatchGAN scale in D's own step, gen_train._d_f32) */
int64_t hrv_conv_s2_packed_bytes(int32_t mode, int32_t K, int32_t cols);   /* -1: shape not served */
int hrv_conv_s2_supported(int32_t mode, int32_t K, int32_t cols, int32_t Cph, int32_t N, int32_t Ho, int32_t Wo);
int hrv_conv_s2_pack_dev(int32_t mode, const float* w, int32_t K, int32_t cols, int32_t Cph, const float* sigma, float wscale,
                         void* out, hrv_stream_t stream);
/* up to 8 weights in one launch (a PatchGAN pass packs three forward / two data-gradient weights per scale) */
typedef struct hrv_s2_pack_job {
  int32_t mode_flags, K, cols, Cph;
  const float* w; const float* sigma; float wscale; int32_t _pad;
  void* out;
} hrv_s2_pack_job_t;
int hrv_conv_s2_pack_multi_dev(int32_t n, const hrv_s2_pack_job_t* jobs, hrv_stream_t stream);
int hrv_conv_s2_bf16(const hrv_conv_s2_t* d, hrv_stream_t stream);
/* bf16-storage companions of hrv_conv_s2_bf16 (the PatchGAN with bf16-stored feature maps): the space-to-depth image of model0's
 * input written in bf16 (cf. hrv_space_to_depth2_nhwc_f32), InstanceNorm2d(affine=False) + LeakyReLU written in bf16
 * (cf. hrv_instnorm_apply_nhwc_f32; network_generator.py:268-269), x *= s_host * (s_dev ? s_dev[0] : 1) over a bf16 loss gradient
 * (cf. hrv_scale_f32), and out[r][w] = w < W ? in[r][w] : 0 for a dY whose width the quad-staged weight gradient needs padded to 4. */
/* the space-to-depth image of model0's input (cf. hrv_space_to_depth2_nhwc_f32) in bf16 over Hp x Wp cells (>= H/2 x W/2; cells and
 * sub-pixels outside the image are zeros: with a one-cell border model0
 * is a 'same' 2x2 convolution, a shape hrv_conv2d_wgrad's LDS-DMA kernel serves), optionally as [hi | lo | hi] */
int hrv_space_to_depth2_cells_bf16(const float* in, int32_t N, int32_t H, int32_t W, int32_t C, int32_t in_cstride, int32_t in_coff,
                                   int32_t Hp, int32_t Wp, int32_t split3, uint16_t* out, hrv_stream_t stream);
int hrv_instnorm_apply_nhwc_bf16out(const float* x, int32_t N, int32_t H, int32_t W, int32_t C, int32_t cstride, int32_t coff,
                                    const float* mean, const float* rstd, int32_t act, float act_slope, uint16_t* out,
                                    int32_t out_cstride, int32_t out_coff, hrv_stream_t stream);
int hrv_scale_bf16(uint16_t* x, int64_t n, float s_host, const float* s_dev, hrv_stream_t stream);
/* out[p] = [hi(x[p]) | bf16(x[p] - hi(x[p])) | hi(x[p])] (3 C bf16 channels, dense) of an fp32 NHWC slice: see HRV_S2_SPLIT3 */
int hrv_split3_nhwc_bf16(const float* x, int64_t npix, int32_t C, int32_t cstride, int32_t coff, uint16_t* out, hrv_stream_t stream);
int hrv_pad_width_nhwc_bf16(const uint16_t* in, int64_t rows, int32_t W, int32_t C, int32_t Wp, uint16_t* out, hrv_stream_t stream);

/* ---- evaluation metrics (evaluate.py; metrics.hip) ---- */
/* PIL Image.convert('L') of packed RGB uint8 pixels, bit-exact: (r*19595 + g*38470 + b*7471 + 0x8000) >> 16 */
int hrv_rgb_to_gray_u8(const uint8_t* rgb, int64_t npix, uint8_t* gray, hrv_stream_t stream);
/* bytes of the per-block partials hrv_pair_stats_u8 needs */
int64_t hrv_pair_stats_workspace_bytes(int32_t B, int32_t H, int32_t W);
/* B pairs of RGB uint8 [B,H,W,3] (H, W >= 11): ssim[b] = skimage structural_similarity of the PIL gray images (evaluate.py:67:
 * data_range=255, gaussian_weights=True -- sigma 1.5, truncate 3.5, reflect border --, use_sample_covariance=False, mean over the
 * map cropped by 5 pixels), mse[b] = sum((gt - pred)^2) / (255^2 * 3HW) (evaluate.py:78-80; the sum is exact).  valid[b] == 0
 * (valid may be NULL): pair skipped, both outputs 0.  Fixed-order reductions: bit-identical across runs. */
int hrv_pair_stats_u8(const uint8_t* gt, const uint8_t* pred, const int32_t* valid, int32_t B, int32_t H, int32_t W,
                      void* workspace, int64_t workspace_bytes, double* ssim, double* mse, hrv_stream_t stream);
/* LPIPS input (evaluate.py:30-33 + the v0.1 ScalingLayer, networks_basic.py:94-101): uint8 [N,H,W,3] -> fp32 NHWC [N,H,W,4]
 * ((u/255 - 0.5)/0.5 - shift[c]) / scale[c], channel 3 zero; shift3 / scale3 are host arrays */
int hrv_lpips_prep_u8(const uint8_t* rgb, int32_t N, int32_t H, int32_t W, const float* shift3, const float* scale3, float* out,
                      hrv_stream_t stream);
/* the same from fp32 NCHW [N,3,H,W] (PerceptualLoss.forward); normalize != 0: 2x - 1 first (eval_models/__init__.py:36-38) */
int hrv_lpips_prep_nchw_f32(const float* x, int32_t N, int32_t H, int32_t W, int32_t normalize, const float* shift3,
                            const float* scale3, float* out, hrv_stream_t stream);
/* MaxPool2d(3, 2) (floor mode, no padding) over dense NHWC fp32 [N,H,W,C], C % 4 == 0 -> [N,(H-3)/2+1,(W-3)/2+1,C] */
int hrv_maxpool3x3s2_nhwc_f32(const float* x, int32_t N, int32_t H, int32_t W, int32_t C, float* y, hrv_stream_t stream);
/* one LPIPS tap: feature maps of the two images (NHWC fp32, pixel stride cstride, pair b at + b*HW*cstride) and the 1x1 lin weights */
typedef struct {
  const float* f0; const float* f1; const float* lin;
  int32_t HW; int32_t C; int32_t cstride; int32_t _pad;
} hrv_lpips_tap_t;
/* out[b] = sum over taps k (in order) of mean_pixels sum_c lin_k[c] * (f0/(||f0||+1e-10) - f1/(||f1||+1e-10))^2  (PNetLin.forward,
 * networks_basic.py:60-86, spatial=False); ntaps <= 8, taps is a host array */
int hrv_lpips_head_f32(const hrv_lpips_tap_t* taps, int32_t ntaps, int32_t B, float* out, hrv_stream_t stream);

/* ---- Inception-v3 (evaluate.py's Inception Score; inception.hip).  The convolutions run on hrv_conv2d_nhwc_f32. ---- */
/* The network's 3x3 pools over channels [coff, coff + C) of NHWC fp32 tensors (C, cstride, coff multiples of 4), so a pool reads
 * a slice and writes a slice of a concatenation.  mode 0: max, stride 2, no padding, floor -> [N,(H-3)/2+1,(W-3)/2+1,C] (exact);
 * mode 1: average, stride 1, padding 1, always divided by 9 (F.avg_pool2d's count_include_pad=True) -> [N,H,W,C], the nine values
 * added in double and rounded once; mode 2: the same sum divided by the number of taps inside the image (count_include_pad=False:
 * 4, 6 or 9); mode 3: max, stride 1, padding 1 -> [N,H,W,C], padding never wins (exact).  Modes 2 and 3 are the pooled branches of
 * the FID variant of the network.  Channels of `y` outside the slice are not touched.  x and y must not overlap. */
int hrv_pool3x3_nhwc_f32(const float* x, int32_t N, int32_t H, int32_t W, int32_t C, int32_t x_cstride, int32_t x_coff, int32_t mode,
                         float* y, int32_t y_cstride, int32_t y_coff, hrv_stream_t stream);
/* The classifier head over the last feature map feat [N,HW,cstride] (channels [0, C)): pooled[n][c] = mean over the HW pixels
 * (workspace, N*C floats), logits[n][k] = sum_c pooled[n][c] * fc_w[k][c] + fc_b[k] (fc_b may be NULL), and -- where probs is not
 * NULL -- probs[n][:] = softmax(logits[n][:]).  Fixed summation orders that do not depend on N: an image's row has the same bits
 * in every batch and on every run. */
int hrv_inception_head_f32(const float* feat, int32_t N, int32_t HW, int32_t C, int32_t cstride, const float* fc_w, const float* fc_b,
                           int32_t K, float* pooled, float* logits, float* probs, hrv_stream_t stream);

/* The FID input in one pass (pytorch-fid's F.interpolate(x / 255, size=(Ho, Wo), mode='bilinear', align_corners=False), then 2v - 1):
 * uint8 [N,H,W,3] of any size -> fp32 NHWC [N,Ho,Wo,4], channel 3 zero.  Source coordinate max(0, (o + 0.5) * in / out - 0.5), upper
 * neighbour clamped to the last row / column, no antialiasing; evaluated in double on the pixel values and rounded to fp32 once (a
 * constant image c gives exactly the fp32 nearest to 2c/255 - 1). */
int hrv_fid_prep_u8(const uint8_t* rgb, int32_t N, int32_t H, int32_t W, int32_t Ho, int32_t Wo, float* out, hrv_stream_t stream);
/* The first stage of the head on its own: pooled[n][c] = mean over the HW pixels of feat [N,HW,cstride] (channels [0, C)), in pixel
 * order, fp32 [N,C] -- the 2048-wide FID feature.  The same bits as the head's workspace. */
int hrv_inception_pool_f32(const float* feat, int32_t N, int32_t HW, int32_t C, int32_t cstride, float* pooled, hrv_stream_t stream);

/* ---- feature statistics of FID / KID in float64 on the matrix cores (feat_stats.hip) ---- */
/* C[i][j] = epi(sum_k A[i][k] * B[j][k]), i < M, j < N: A [M][lda], B [N][ldb] row-major with k contiguous, both fp32
 * (operands_f64 == 0) or both fp64; products and sums in fp64 on v_mfma_f64_16x16x4_f64 in ascending k; C fp64 [M][ldc].  No atomics,
 * no split-K: an element does not depend on the grid.  Any M, N, K >= 1.  epilogue 0 (linear): s * param; 1 (poly3):
 * t = s / param + 1, (t * t) * t -- KID's polynomial kernel with param = the feature width.  symmetric != 0 (needs B == A, N == M):
 * only tiles on and above the diagonal are computed and each element is written to (i, j) and (j, i), so C is bitwise symmetric. */
int hrv_gemm_nt_f64(const void* A, const void* B, int32_t operands_f64, int32_t M, int32_t N, int32_t K, int64_t lda, int64_t ldb,
                    int32_t epilogue, double param, int32_t symmetric, double* C, int64_t ldc, hrv_stream_t stream);
/* mean[c] = (sum over the n rows of x fp32 [n][D], in row order, in fp64) / n */
int hrv_feat_mean_f64(const float* x, int32_t n, int32_t D, double* mean, hrv_stream_t stream);
/* xt fp64 [D][n]: xt[c][r] = (double)x[r][c] - mean[c] */
int hrv_feat_center_t_f64(const float* x, const double* mean, int32_t n, int32_t D, double* xt, hrv_stream_t stream);
/* KID's subset sums: Kxx fp64 [nx][nx], Kyy [ny][ny], Kxy [nx][ny] (dense), ix / iy int32 [S][m] device arrays of row numbers
 * (unsorted, no repeats; an index outside its matrix is not read and turns the sum into NaN).  out fp64 [S][3] = (sum of
 * Kxx[ix,ix] off the diagonal, sum of Kyy[iy,iy] off the diagonal, sum of Kxy[ix,iy]), gathered and added in a fixed order. */
int hrv_kid_subset_sums_f64(const double* Kxx, int32_t nx, const double* Kyy, int32_t ny, const double* Kxy, const int32_t* ix,
                            const int32_t* iy, int32_t S, int32_t m, double* out, hrv_stream_t stream);

/* ---- nearest-neighbour manifold statistics in float64: precision / recall / density / coverage (manifold.hip) ---- */
/* All four: no atomics, nothing that depends on the grid, results bit-identical from run to run; null pointers and bad extents
 * return non-zero before anything is launched. */
/* out[i] = sum over c < D of (double)x[i][c]^2, i < n: x fp32 [n][ld] (ld >= D), out fp64 [n].  Lane l of the row's wave adds
 * columns l, l + 64, ... in ascending order; the 64 partial sums meet in a fixed butterfly (32, 16, 8, 4, 2, 1 lanes apart). */
int hrv_row_sqnorm_f64(const float* x, int32_t n, int32_t D, int64_t ld, double* out, hrv_stream_t stream);
/* out[i][j] = max(0, (normX[i] + normY[j]) - 2 * sum_c X[i][c] * Y[j][c]), i < nx, j < ny: X fp32 [nx][ldx], Y fp32 [ny][ldy] with c
 * contiguous (ldx, ldy >= D), normX fp64 [nx], normY fp64 [ny] (hrv_row_sqnorm_f64 of the same rows), out fp64 [nx][ldo] (ldo >= ny).
 * Products and sums in fp64 on v_mfma_f64_16x16x4_f64 in ascending c, as in hrv_gemm_nt_f64; any nx, ny, D >= 1.  self_offset >= 0
 * (needs self_offset + nx <= ny): the element j == self_offset + i of every row i is written as +inf -- the row's own entry when X
 * is the slab of Y that starts at row self_offset.  self_offset == -1: nothing is replaced. */
int hrv_sqdist_nt_f64(const float* X, const float* Y, int32_t nx, int32_t ny, int32_t D, int64_t ldx, int64_t ldy,
                      const double* normX, const double* normY, int64_t self_offset, double* out, int64_t ldo, hrv_stream_t stream);
/* The largest k hrv_row_kth_f64 serves: a compile-time constant of the library, 16. */
int hrv_row_kth_max(void);
/* out[i] = the k-th smallest (1-based, counted with multiplicity, so defined regardless of ties) of d[i][0 .. n), i < rows: d fp64
 * [rows][ld] (ld >= n), out fp64 [rows]; 1 <= k <= min(hrv_row_kth_max(), n).  +inf sorts last: with fewer than k finite entries the
 * result is +inf.  NaN entries are passed over. */
int hrv_row_kth_f64(const double* d, int32_t rows, int32_t n, int64_t ld, int32_t k, double* out, hrv_stream_t stream);
/* cnt[i] (int32) = #{ j < n : d[i][j] < r_col[j] } (strict) and dmin[i] (fp64) = min over j < n of d[i][j], i < rows: d fp64
 * [rows][ld] (ld >= n), r_col fp64 [n].  Either of cnt, dmin may be NULL (not both).  An integer sum and a minimum: exact in any
 * order. */
int hrv_row_ball_f64(const double* d, const double* r_col, int32_t rows, int32_t n, int64_t ld, int32_t* cnt, double* dmin,
                     hrv_stream_t stream);

/* ---- validation passes of the training scripts (validate.hip) ---- */
/* The counts behind train_condition.py's iou_metric (:18-36), per sample, in one launch: seg fp32 NCHW [N,13,h,w] (raw logits), cm
 * fp32 [N,1,h,w] (may be NULL when comp == 0), label fp32 NCHW [N,13,h,w] (one-hot).  comp 0: no_composition; 1: detach (channel 3
 * times cm > 0.5); 2: warp_grad (channel 3 times cm).  pred = softmax_c(seg * mask) > 0.5 (strict; fp32: subtract the channel
 * maximum, expf, sum in channel order, divide) over all 13 channels and pixels.  out int64 [N,3] = (count of pred && label == 1,
 * count of pred, count of label == 1); the entry zeroes out[0 .. 3N) in-stream first and adds with integer atomics, so the result
 * does not depend on what the buffer held or on scheduling. */
int hrv_seg_iou_nchw_f32(const float* seg, const float* cm, const float* label, int32_t N, int32_t h, int32_t w, int32_t comp,
                         int64_t* out, hrv_stream_t stream);
/* LPIPS input with the resize folded in: in0, in1 fp32 NCHW [N,3,H,W] -> out fp32 NHWC [2N,Ho,Wo,4] (in0's images first), each
 * bilinearly resampled (align_corners=False, no antialiasing) and passed through (v - shift[c]) / scale[c] (2v - 1 first when
 * normalize != 0), channel 3 zero: bit for bit hrv_resize_nchw_f32 followed by hrv_lpips_prep_nchw_f32, in one launch. */
int hrv_lpips_prep_resize_nchw_f32(const float* in0, const float* in1, int32_t N, int32_t H, int32_t W, int32_t Ho, int32_t Wo,
                                   int32_t normalize, const float* shift3, const float* scale3, float* out, hrv_stream_t stream);

/* ---- image grids of the scripts (viz.py; viz.hip) ---- */
#define HRV_VIZ_MAX_PANELS 16
#define HRV_VIZ_MAX_CLASSES 20
enum { HRV_VIZ_SIGNED = 0, HRV_VIZ_UNIT = 1, HRV_VIZ_SEGMAP = 2 };   /* hrv_viz_panel_t.kind */
enum { HRV_VIZ_ROUND = 0, HRV_VIZ_TRUNC = 1 };                       /* quant */
/* One panel of a grid: an fp32 view of N x H x W pixels with C channels, addressed in ELEMENTS as
 * ptr[n * sn + y * sy + x * sx + c * sc] -- NCHW tensors and channel slices of them, NHWC slices, a mask broadcast over the channels
 * (sc == 0) and one sample shown in every grid (sn == 0) need no copy.  kind SIGNED: v = x * 0.5 + 0.5; UNIT: v = x (both C == 3,
 * or C == 1: the one channel is shown as grey); SEGMAP: the index of the first maximum over the C channels (1 <= C <= 20, as
 * np.argmax), shown in the 20-colour palette of the reference's utils.visualize_segmap.  Where sc == 1, ptr is 16-byte aligned and
 * sn, sy, sx are multiples of 4, a pixel is read as float4 groups: the C channels rounded up to a multiple of 4 must then be
 * readable (an NHWC tensor whose channel stride is a multiple of 4); what lies behind channel C - 1 is never looked at. */
typedef struct {
  const float* ptr;
  int64_t sn, sy, sx, sc;
  int32_t C;
  int32_t kind;
} hrv_viz_panel_t;
/* N grids of `npanels` panels in one launch: out uint8 [N,Hg,Wg,3] (4-byte aligned), laid out as torchvision's make_grid with
 * pad_value 0 does: xmaps = min(nrow, npanels), ymaps = ceil(npanels / xmaps), Hg = ymaps * (H + padding) + padding, Wg = xmaps *
 * (W + padding) + padding, panel k at row (k / xmaps) * (H + padding) + padding, column (k % xmaps) * (W + padding) + padding;
 * borders and the unfilled cells of the last row are 0; npanels == 1 gives the bare panel [N,H,W,3].  SIGNED / UNIT values become
 * bytes by quant ROUND: (uint8) clamp(v * 255 + 0.5, 0, 255) with the product and the sum rounded separately (torchvision
 * save_image; not round-half-even), or TRUNC: (uint8) clamp(v * 255, 0, 255) (utils.save_images, tensorboard); SEGMAP bytes are the
 * palette's.  Inputs are assumed finite.  `panels` is a host array: it travels in the kernel arguments. */
int hrv_viz_grid_u8(const hrv_viz_panel_t* panels, int32_t npanels, int32_t nrow, int32_t padding, int32_t N, int32_t H, int32_t W,
                    int32_t quant, uint8_t* out, hrv_stream_t stream);

/* ---- R1 gradient penalty of the PatchGAN by a tangent pass (r1.py; r1.hip) ----
 * InstanceNorm + LeakyReLU under a forward-mode tangent, per (sample, channel) over P = H * W pixels:
 *     y = (x - mean) * rstd;  f = lrelu(y);  tangent t of x:  ydot = rstd * (t - mean_P(t) - y * mean_P(y t));  fdot = lrelu'(y) * ydot
 * (ydot is what hrv_spade_norm_bwd_nhwc_f32 computes for dout = t without an activation: the Jacobian is symmetric).  The two
 * launches below are the REVERSE of that pair of maps.  With df the adjoint of fdot and q = lrelu'(f) * df:
 *     tbar = rstd * (q - mean(q) - y * mean(y q))                                          the adjoint of t
 *     A = sum(q t) - P mean(q) mean(t);  B = P mean(y q) mean(y t);  w = q mean(y t) + t mean(y q)
 *     cbar = -(rstd^2 / P) (A - B) y - rstd^2 (w - mean(w) - y mean(y w)) (+ cin)          the tangent path's adjoint of x
 *     mean(w) = mean(q) mean(y t) + mean(t) mean(y q);  mean(y w) = 2 mean(y q) mean(y t)
 * hrv_instnorm_jvp_stats_nhwc_f32: record[n][c][0..4] = sum q, sum t, sum y q, sum y t, sum q t (fp64; every product and sum in
 *   fp64 from the fp32 operands).  Pixel slabs as hrv_instnorm_stats_nhwc_f32 (a function of H * W alone), one chain per thread in
 *   pixel order, rows and slabs combined in a fixed order, no atomics: the same operands give the same bits in every run.
 *   workspace: hrv_instnorm_jvp_workspace_elems doubles.
 * hrv_instnorm_jvp_bwd_nhwc_f32: the element-wise pass; reads the record, writes tbar and cbar (fp64 arithmetic, one rounding to
 *   fp32 per output).  cin (nullable): an adjoint of x that arrives by another path (the ordinary InstanceNorm backward of the
 *   primal feature's adjoint), added in fp64 before that rounding.  P = 1 gives y = 0, tbar = 0 and cbar = cin, all finite.
 * C is the padded channel count (C % 4 == 0; mean / rstd are [N][C]); every tensor is a channel slice [coff, coff + C) of an NHWC
 * tensor with pixel stride cstride (both multiples of 4, base pointers 16-byte aligned).  tbar / cbar must not alias an input. */
typedef struct {
  const float* x;     /* the InstanceNorm input c */
  const float* mean;  const float* rstd;
  const float* f;     /* lrelu(y): its sign is the mask */
  const float* t;     /* tangent of x */
  const float* df;    /* adjoint of fdot */
  const float* cin;   /* nullable */
  float* tbar;  float* cbar;
  double* record;     /* [N][C][5] */
  double* workspace;  /* the stats launch only; the element-wise launch ignores it (may be NULL) */
  int32_t N, H, W, C;
  int32_t x_cstride, x_coff, f_cstride, f_coff, t_cstride, t_coff, df_cstride, df_coff, cin_cstride, cin_coff;
  int32_t tbar_cstride, tbar_coff, cbar_cstride, cbar_coff;
  float slope;
  int32_t reserved;
} hrv_instnorm_jvp_t;
int64_t hrv_instnorm_jvp_workspace_elems(int32_t N, int32_t H, int32_t W, int32_t C);
int hrv_instnorm_jvp_stats_nhwc_f32(const hrv_instnorm_jvp_t* d, hrv_stream_t stream);
int hrv_instnorm_jvp_bwd_nhwc_f32(const hrv_instnorm_jvp_t* d, hrv_stream_t stream);
/* The seed of the tangent pass.  d_in [N][H][W][Cp] (dense, Cp % 4 == 0): the gradient of sum_n S_n w.r.t. the assembled input
 * [parse (Ca) ; image (Cb) ; pad].  v (same shape) = d_in * (1.0f / N) on the image channels [Ca, Ca + Cb) and exactly 0 on every
 * other channel, whatever d_in holds there (a select, not a product).  part: double [N][hrv_r1_seed_slots()], the per-slot sums of
 * squares of the image channels (fp64; pixel i of a sample belongs to slot (i / 256) % slots; fixed order, no atomics).  The same
 * call then runs one finalize block: sums[n] = sum of the slots (fixed tree), out[0] = penalty = (sum_n sums[n]) / N and
 * out[1] = gamma / 2 * penalty, both rounded once to fp32.  Nothing is read back. */
int hrv_r1_seed_slots(void);
int hrv_r1_seed_nhwc_f32(const float* d_in, int32_t N, int32_t H, int32_t W, int32_t Cp, int32_t Ca, int32_t Cb, float gamma,
                         float* v, double* part, double* sums, float* out, hrv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* HRVITON_HIP_H */
