/* sbc_hip.h -- C ABI of libsbc_hip.so: the annealed-Langevin MIMO channel-estimation hot path of
 * utcsilab/score-based-channels as hand-written HIP kernels for gfx950 (MI355X).
 *
 * The reference has no FFI of its own: its operator boundary is the PyTorch call
 *     score = diffuser(current_real, labels)                 (src/score_based_channels/test_score.py:151)
 * on an NCSNv2Deepest nn.Module (ncsnv2/models/ncsnv2.py:198-300) plus the tensor expressions of the
 * sampling loop around it (test_score.py:118-171, copied in tune_hparams_score.py:100-148).  This
 * library replaces exactly that: the host side (Python, score_based_channels_amd/) builds a *plan* -- an
 * ordered list of fused operator launches over NHWC float32 device buffers it owns -- and the library
 * executes it on a HIP stream.  One plan = one score evaluation, optionally followed by the
 * data-consistency + Langevin update + NMSE of one step, so that a whole trajectory is
 * sbc_plan_run(plan, stream, n_steps) with no host synchronisation (the reference syncs every step,
 * test_score.py:137,170).
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer borrowed for the duration of the
 *     call / the lifetime of the plan (buffers stay owned by the caller, normally torch tensors);
 *   - activations are NHWC float32: x[n][h][w][c]; a complex64 [B][Nt][Nr] tensor IS a 2-channel NHWC
 *     tensor (re, im interleaved), which removes the reference's real/complex view copies
 *     (test_score.py:149,153-154);
 *   - every function returns 0 on success or a negative sbc_status; sbc_last_error() gives the message of
 *     the calling thread's last failure.  Nothing throws across the ABI.  Launches are asynchronous on the
 *     given stream (pass torch.cuda.current_stream().cuda_stream); no hidden device synchronisation
 *     except in the functions documented as synchronising.
 *
 * Beside the plan interface the library carries the other estimators of the paper's Fig. 5c, each a self-contained group of calls
 * with its own section below: the lifted-DFT l1 solver and regularised least squares (sbc_l1_lifted_run, sbc_ls_regularized), Learned
 * D-AMP (sbc_ldamp_*) and the WGAN latent optimisation (sbc_wgan_*: generator forward, backward and Adam on the latents; sbc_wgan_trainer_*:
 * the critic and generator iterations that train that generator).  The
 * network baselines keep their activations planar, [N][C][H][W] float32, in a workspace the caller owns.
 */
#ifndef SBC_HIP_H
#define SBC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SBC_ABI_VERSION 16

typedef enum sbc_status {
    SBC_OK = 0,
    SBC_ERR_INVALID = -1,      /* bad argument / unsupported shape */
    SBC_ERR_HIP = -2,          /* a HIP runtime call failed (message has hipGetErrorString) */
    SBC_ERR_UNSUPPORTED = -3   /* no kernel instantiation for this (cin, cout, ksize) */
} sbc_status;

/* Operator kinds.  Reference counterparts (file:line under /root/reference): */
typedef enum sbc_op_kind {
    SBC_OP_BEGIN_CONV = 1,   /* h = 2x-1; begin_conv 2->ngf 3x3 + bias          ncsnv2.py:270-275            */
    SBC_OP_INORM_STATS = 2,  /* InstanceNorm2dPlus statistics -> (mu, scale, shift) normalization.py:163-176 */
    SBC_OP_CONV = 3,         /* nn.Conv2d 1x1 / 3x3 / dilated 3x3 with fused prologue+epilogue  layers.py:28-60,
                                ResidualBlock :443-456, RCUBlock :126-134, CRPBlock :76-83, MSFBlock :178-184,
                                ConvMeanPool :309-313                                                        */
    SBC_OP_MAXPOOL5 = 4,     /* nn.MaxPool2d(5, stride 1, pad 2) (+ELU of the input)  layers.py:69,77-80      */
    SBC_OP_END_CONV = 5,     /* normalizer -> ELU -> end_conv ngf->2 -> / sigma   ncsnv2.py:291-298           */
    SBC_OP_LANGEVIN = 6,     /* P^H(PX-Y), noise, Langevin update, NMSE           test_score.py:156-170       */
    SBC_OP_STEP_INC = 7,     /* advance the device-side step counter (trailing_idx, test_score.py:171)        */
    SBC_OP_MEASURE = 8,      /* Y = P H + sqrt(noise) n                           test_score.py:122-124       */
    /* --- denoising-score-matching training step: ncsnv2/losses/dsm.py:6-32,
     *     train_score.py:145-173.  Reverse-mode counterparts of the operators above; see "Training operators". */
    SBC_OP_DSM_PERTURB = 9,  /* x~ = x + sigma_b z, z ~ N(0,1)                    dsm.py:14-17                */
    SBC_OP_DSM_LOSS = 10,    /* 1/2 |s + z/sigma|^2 sigma^p per sample (+ d/ds)   dsm.py:19-32                */
    SBC_OP_GRAD_ADD = 11,    /* out (+)= grad [* ELU'(in)]                        backward of +, of nn.ELU    */
    SBC_OP_INORM_BWD = 12,   /* backward of InstanceNorm2dPlus (+ ELU)            normalization.py:163-176    */
    SBC_OP_MAXPOOL5_BWD = 13,/* backward of nn.MaxPool2d(5,1,2) (+ ELU of input)  layers.py:69,77-80          */
    SBC_OP_UPSAMPLE_BWD = 14,/* adjoint of the bilinear(align_corners) resize     layers.py:182               */
    SBC_OP_POOL_BWD = 15,    /* adjoint of the 2x2 mean pool of ConvMeanPool      layers.py:311-312           */
    SBC_OP_CONV_WGRAD = 16,  /* d loss / d weight, d bias of an SBC_OP_CONV       layers.py:28-60             */
    SBC_OP_PACK_WEIGHT = 17, /* torch-layout weight (device) -> split-bf16 fragments, optionally of the adjoint conv */
    SBC_OP_END_CONV_BWD = 18,/* backward of SBC_OP_END_CONV up to the ELU output  ncsnv2.py:291-298           */
    SBC_OP_BEGIN_CONV_BWD = 19, /* weight / bias gradient of SBC_OP_BEGIN_CONV    ncsnv2.py:270-275           */
    SBC_OP_ADAM_EMA = 20,    /* torch.optim.Adam step + EMAHelper.update          losses/__init__.py:3-7, ema.py:17-22 */
    SBC_OP_CONV_PAIR = 21,   /* one RCU block in one launch: out = x + conv2(ELU(conv1(ELU(x))))   layers.py:126-134;
                                32 (or, fp16 weights, 64) channels, 3x3, no bias; the intermediate stays in LDS
                                (csrc/conv_pair.hip)                                                                  */
    SBC_OP_CONV_POOL = 22,   /* (ABI 11) one CRP stage in one launch: out = conv3x3(ELU?(MaxPool5x5(x))) [+ (res2 + ELU?(res1))]
                                layers.py:76-83; replaces an SBC_OP_MAXPOOL5 record and the SBC_OP_CONV that reads it: the
                                pooled tensor never exists in memory (csrc/conv_pair.hip: conv_pool_kernel)                  */
    SBC_OP_RES_BLOCK = 23,   /* (ABI 12) one ResidualBlock without resampling in one launch:
                                out = x + conv2(ELU(norm2(conv1(ELU(norm1(x))))))   layers.py:443-456, normalization.py:150-176;
                                32 channels, 64 x 16 samples: a workgroup owns a whole sample, so it forms the InstanceNorm++
                                statistics of the intermediate itself (csrc/conv_res.hip)                                    */
    SBC_OP_CONV_DOWN = 25,   /* (ABI 13) the tail of a downsampling ResidualBlock in one launch (layers.py:443-456 with ConvMeanPool :309-313):
                                out = meanpool2(conv3x3(ELU(norm(in))) + bias) + meanpool2(conv1x1(res1) + bias2), as a 4x4 stride-2 and a
                                2x2 stride-2 direct convolution with the pooled filters (weight_split = sbc_pack_conv_weight_pooled_f16x2 of the
                                3x3 weight, weight2_split = the same of the 1x1 shortcut weight); in = conv1's output, res1 = the block's input,
                                both [B][H][W][cin], stats = the norm's (mu, scale, shift); 32 -> 64 channels at W = 16, 64 -> 64 at W = 8,
                                H a multiple of 16; SBC_CONV_F16X2 only (csrc/conv_down.hip).  Calibration only (no kernel reads them, NULL is
                                fine): weight / weight_wino_split = the UNPOOLED direct (sbc_pack_conv_weight_f16x2) and Winograd f16x2 forms of the
                                3x3 layer, weight_wino = the unpooled direct f16x2 form of the 1x1 shortcut -- sbc_f16x2_calibrate writes the two
                                layers' activation scales into those trailers too (a host that binds the same weight buffer at a size where the
                                block is not down-fusable runs the unfused launches with the same scales)                                  */
    SBC_OP_CHAIN = 24        /* (ABI 13) a CHAIN of RCU blocks, CRP blocks and ResidualBlocks in ONE launch, for the low
                                resolution levels (8 x 2 samples of 64 or 128 channels, 16 x 4 samples of 64, 32 x 8 samples of 32 or
                                64; layers.py:76-83,126-134,234-249,443-456): a workgroup owns eight (four, one or two) samples, the
                                running tensor x stays in registers between the blocks and the convolution operands in LDS; only
                                the filters stream (csrc/conv_chain.hip).  ext = sbc_chain                                    */
} sbc_op_kind;

/* sbc_op.flags for SBC_OP_CONV / SBC_OP_MAXPOOL5 */
#define SBC_PRO_ELU      0x001  /* apply ELU to the input while staging it                                  */
#define SBC_PRO_NORM     0x002  /* apply (x - mu) * scale + shift from `stats` first (InstanceNorm++)       */
#define SBC_PRO_NORM_SELF 0x004 /* (ABI 10) with SBC_PRO_NORM, 3x3 convolutions on the matrix-core kernels (weight_split set), images of at most 64
                                   pixels (H*W a power of two): the launch computes the InstanceNorm++ statistics of its input
                                   ITSELF -- a workgroup's tile holds whole samples there -- and `stats` points at the norm's
                                   parameters [3][cin] = (alpha | gamma | beta) instead of at the output of an
                                   SBC_OP_INORM_STATS launch, which then does not exist (normalization.py:163-176)          */
#define SBC_PRO_ELU_ACC  0x20000 /* (ABI 11) with SBC_PRO_ELU: evaluate ELU with fp32's relative accuracy for small negative inputs too (a
                                   polynomial below |x| = 1/32 instead of exp(x) - 1, whose absolute error of 6e-8 is 6e-5 of an
                                   activation of -1e-3): ten vector instructions per value instead of four.  The Python host sets
                                   it in the exact modes (conv_mode 0 / 1); in conv_mode 3 the layer's weight trailer asks for it
                                   when sbc_f16x2_calibrate finds the layer's input maximum below 0.5                       */
#define SBC_EPI_RES1_ELU 0x010  /* ELU the res1 operand before adding (CRP: x = act(x))                    */
#define SBC_EPI_POOL     0x020  /* 2x2 mean pool of (conv + bias), then + res1 (ConvMeanPool)               */
#define SBC_EPI_UP       0x040  /* + bilinear(align_corners) resize of `up` [B][up_h][up_w][cout] (MSF)     */
#define SBC_EPI_ELUGRAD  0x080  /* reverse pass (split-bf16 kernels, no pool): out = conv * ELU'(res2) [+ res1]; res2 = the
                                   forward input the ELU was applied to, res1 = the gradient collected so far (may be
                                   `out` itself: every element is read and written by the same thread)              */
#define SBC_BWD_ACCUM     0x200  /* training operators: add to `out` instead of overwriting it (a tensor with several
                                   consumers collects one gradient term per consumer)                            */
#define SBC_PACK_ADJOINT  0x400  /* SBC_OP_PACK_WEIGHT: pack w'[ci][co][kh][kw] = w[co][ci][k-1-kh][k-1-kw], the weight of
                                   the adjoint (input-gradient) convolution, which then runs as an ordinary SBC_OP_CONV */
#define SBC_OP_SIDE       0x800  /* any kind, inside a plan: this launch may overlap the launches that follow it.  The plan
                                   runs it on a stream of its own that first waits for everything issued before it; side
                                   launches keep their order among themselves.  The caller guarantees that no later launch
                                   writes what it reads or reads what it writes before the next SBC_OP_JOIN             */
#define SBC_OP_JOIN       0x1000 /* this launch (and everything after it) waits for all side launches issued so far; the
                                   end of the plan always joins                                                       */
#define SBC_PACK_WINOGRAD 0x2000 /* SBC_OP_PACK_WEIGHT: the Winograd F(2x2,3x3) form (sbc_pack_conv_weight_winograd_split layout) of a
                                   3x3 weight; combines with SBC_PACK_ADJOINT                                          */
#define SBC_PRO_NORM_MOMENTS 0x4000 /* INORM_STATS: `in` holds the tensor's TILE MOMENTS [B][H*W/128][cin][2] = (mean, sum (x - mean)^2) of
                                      each 128-pixel tile, written by the launch that produced the tensor (SBC_EPI_MOMENTS_OUT);
                                      H, W, cin describe the tensor.  The statistics launch then reads a few KB per sample
                                      instead of the tensor (32 or, ABI 10, 64 channels)                                   */
#define SBC_EPI_MOMENTS_OUT 0x8000 /* CONV (Winograd split kernels, 32 or -- ABI 10 -- 64 output channels, whole 128-pixel tiles, no
                                      pool) and BEGIN_CONV: also write the tile moments of the output to `aux` [B][H*W/128][cout][2] */
#define SBC_CONV_F16W    0x100  /* fp16 weights (BASELINE config 5): `weight_split` / `weight_wino_split` hold ONE
                                   fp16 term per weight (sbc_pack_conv_weight_f16 / _winograd_f16) instead of
                                   three bf16 terms; activations are rounded to fp16 as they enter the matrix
                                   cores (v_mfma_f32_32x32x16_f16), accumulation stays fp32                    */

#define SBC_CONV_F16X2   0x10000 /* fp32-class arithmetic on the fp16 matrix cores: `weight_split` / `weight_wino_split` hold TWO
                                   fp16 terms per (scaled) weight plus a 16-byte trailer with the scales
                                   (sbc_pack_conv_weight_f16x2 / _winograd_f16x2); activations are scaled by the layer's
                                   act_scale (a power of two; sbc_f16x2_calibrate) and split into two fp16 terms as they enter
                                   the matrix cores; three fp16 MFMAs per product block (hh + hl + lh), fp32 accumulation.
                                   Representation error <= 2^-22 per operand while 2^-3 <= |x| act_scale < 16000; outside that
                                   window the device's range flag (sbc_range_flag) is raised instead of returning silently
                                   degraded numbers                                                                       */

/* One fused launch.  Unused fields are 0 / NULL.  Tensor shapes per kind:
 *   BEGIN_CONV  in [B][H][W][2], weight [cout][2][3][3] (torch layout), bias [cout], out [B][H][W][cout]
 *   INORM_STATS in [B][H][W][cin], weight = alpha|gamma|beta [3][cin], out = stats [B][3][cin]
 *   CONV        in [B][H][W][cin], weight = sbc_pack layout [k*k][cin/8][cout/32][64][4], bias [cout] or
 *               NULL, stats [B][3][cin] (PRO_NORM), res1/res2 [B][Ho][Wo][cout] or NULL, up (EPI_UP),
 *               out [B][Ho][Wo][cout] with Ho,Wo = H,W or H/2,W/2 (EPI_POOL).
 *               epilogue:  v = conv + bias;  [POOL: v = mean2x2(v)]
 *                          r = res1 [ELU];  if res2: r = res2 + r;  v = v + r;  [UP: v = v + resize(up)]
 *   MAXPOOL5    in/out [B][H][W][cin]; PRO_ELU applies ELU (monotone, so pooled after or before is equal)
 *   END_CONV    in [B][H][W][cin], stats, weight [2][cin][3][3] (torch layout), bias [2], out [B][H][W][2];
 *               divides by sigmas[labels[b]] if labels != NULL else by sigma_of_step[*step]
 *   LANGEVIN    see sbc_langevin below (passed through `ext`)
 *   CONV_PAIR   in / out [B][H][W][C] (distinct buffers), weight_split + weight2_split, flags = SBC_CONV_F16X2 or
 *               SBC_CONV_F16W; C = 32: W in {8, 16} with H % 8 == 0, or (SBC_CONV_F16W only) W in {32, 64} with H % 4 == 0;
 *               C = 64 (SBC_CONV_F16W only): W = 16 with H % 8 == 0 or W = 32 with H % 4 == 0.  The same numbers as the two CONV records it replaces
 *               (PRO_ELU; PRO_ELU + res1 = in) up to fp32 summation order.
 *   CONV_POOL   in / out [B][H][16][32] (distinct buffers), weight_split (the form of CONV_PAIR), no bias; flags = SBC_CONV_F16X2 or
 *               SBC_CONV_F16W, optionally SBC_PRO_ELU (ELU of the pooled values: pool(ELU(x)) = ELU(pool(x))) and SBC_EPI_RES1_ELU;
 *               res1 / res2 as in CONV (r = res1 [ELU]; if res2: r = res2 + r; out = conv + r); H % 8 == 0.  The same numbers as
 *               the MAXPOOL5 + CONV records it replaces up to fp32 summation order (direct instead of Winograd form).
 *   RES_BLOCK   in / out [B][64][16][32] (distinct buffers); stats = the (mu, scale, shift) table of norm1 [B][3][32] (an INORM_STATS
 *               output); weight_split / bias = conv1, weight2_split / bias2 = conv2 (sbc_pack_conv_weight_f16x2; flags =
 *               SBC_CONV_F16X2); norm2 = alpha | gamma | beta of the second norm [3][32]; with SBC_EPI_MOMENTS_OUT, aux = the output's
 *               tile moments [B][8][32][2] (what a CONV with that flag writes).  The same numbers as the CONV (PRO_NORM | PRO_ELU),
 *               INORM_STATS, CONV (PRO_NORM | PRO_ELU, res1 = in) records it replaces up to fp32 summation order.
 */
typedef struct sbc_op {
    int32_t kind, flags;
    int32_t B, H, W;
    int32_t cin, cout, ksize, dil;
    int32_t up_h, up_w;
    int32_t tag;                 /* free label; sbc_plan_profile times all ops carrying a given tag.  tag 1 = the 3x3 ngf -> ngf
                                    layers at full resolution: they also run under their own kernel symbol so that profilers
                                    report them separately */
    const void* in;
    void* out;
    const void* weight;
    const void* bias;
    const void* stats;
    const void* res1;
    const void* res2;
    const void* up;
    const void* ext;             /* kind-specific extension struct (sbc_langevin / sbc_endconv), host memory,
                                    copied at sbc_plan_create / read during sbc_op_launch */
    const void* weight_wino;     /* CONV, optional: the same 3x3 weight in Winograd F(2x2,3x3) form,
                                    sbc_pack_conv_weight_winograd layout [16][cin/8][cout/32][64][4]; used for
                                    undilated 3x3 convolutions on power-of-two images (2.25x fewer multiplies),
                                    `weight` stays the fallback for every other shape */
    const void* weight_split;    /* CONV, optional: the same weight with every fp32 value split exactly into three
                                    bf16 terms, sbc_pack_conv_weight_split layout [k*k][cin/16][cout/32][3][64][8]
                                    (uint16).  When set, the convolution runs on the bf16 matrix cores as six bf16
                                    MFMAs per fp32 product block with fp32 accumulation (fp32-level accuracy, see
                                    csrc/conv_x3.hip); takes precedence over `weight_wino` and `weight`, which then
                                    may be NULL. */
    const void* weight_wino_split; /* CONV, optional: the Winograd form of a 3x3 weight with every value split into three
                                    bf16 terms, sbc_pack_conv_weight_winograd_split layout [16][cin/16][cout/32][3][64][8]
                                    (uint16): Winograd F(2x2,3x3) with its 16 products on the bf16 matrix cores
                                    (csrc/conv_wx3.hip).  Used for undilated 3x3 convolutions on power-of-two images,
                                    ahead of `weight_split`. */
    /* --- training operators only (ABI 7; NULL / unused on the inference path) --- */
    const void* grad;            /* incoming gradient: d loss / d (this operator's forward output) */
    void* aux;                   /* kind-specific second output or scratch (see "Training operators") */
    void* wgrad;                 /* parameter-gradient output: conv weight in torch layout, or alpha|gamma|beta [3][cin] */
    void* bgrad;                 /* bias-gradient output [cout] or NULL */
    /* --- ABI 9 --- */
    const void* weight2_split;   /* CONV_PAIR: the second convolution's weight in the form `weight_split` holds the first one's
                                    (sbc_pack_conv_weight_f16x2 with SBC_CONV_F16X2, sbc_pack_conv_weight_f16 with SBC_CONV_F16W) */
    /* --- ABI 11 --- */
    void* calib;                 /* NULL.  (Set by sbc_f16x2_calibrate on its private copies of the records: two device floats per
                                    f16x2 convolution that collect max |x| of what the launch stages.) */
    /* --- ABI 12 --- */
    const void* bias2;           /* RES_BLOCK: bias of the second convolution [cout] */
    const void* norm2;           /* RES_BLOCK: alpha | gamma | beta of the second InstanceNorm++ [3][cout] */
    /* --- ABI 13 --- */
    const void* weight2_wino_split; /* CONV_PAIR / RES_BLOCK: the second convolution's Winograd f16x2 form, or NULL.  No kernel of a fused
                                    record reads it (nor `weight_wino_split` there): sbc_f16x2_calibrate writes the layer's activation
                                    scale into the trailer of EVERY form it is handed, so that a host which shares one weight buffer
                                    between array sizes -- fused at one, unfused Winograd at another -- finds the same scale in both */
    /* --- ABI 14: launch lanes of a plan (all zero: the record runs on the run stream in list order, as before) --- */
    int32_t lane;                /* 0 = the stream handed to sbc_plan_run; 1 .. SBC_MAX_LANES-1 = a stream of the library that goes with that
                                    run stream (probed once to sit on another hardware queue; shared by the plans run on it).  Records of one
                                    lane run in list order; records of different lanes are ordered ONLY by the events below (and by the
                                    start and the end of an sbc_plan_run call, which every lane is forked from / joined into) */
    int32_t signal;              /* 0, or an event id 1 .. SBC_MAX_EVENTS: recorded on this record's lane right behind it */
    int32_t wait[2];             /* 0, or event ids this record's lane waits for in front of it; the id must be signalled by a record
                                    EARLIER in the list (of the same iteration).  The host that builds the list owns the hazards: a
                                    record must not write what a concurrently running lane reads or writes (sbc_score_wiring_create shares storage accordingly) */
} sbc_op;
#define SBC_MAX_LANES 4
#define SBC_MAX_EVENTS 64

/* Training operators.  The reverse of a forward record `y = epi(conv(pro(x)))` is built by the host
 * (score_based_channels_amd/train.py) from these pieces; every tensor is NHWC float32 like its forward counterpart, `grad`
 * always has the shape of the forward OUTPUT of the operator being reversed, `out` the shape of its forward INPUT.
 *   DSM_PERTURB   in = samples [B][n] (n = H*W*cin), ext = sbc_dsm; out = samples + sigmas[labels[b]] * z;
 *                 aux = the scaled noise sigma_b * z [B][n] (kept for the loss).  z = ext.noise (standard normal draws,
 *                 replay) or in-kernel Philox keyed by (seed, sample_id[b] or b, offset, element).
 *   DSM_LOSS      in = scores [B][n], grad = scaled noise [B][n], ext = sbc_dsm; out = per-sample loss [B]:
 *                 1/2 * sum_n (s - t)^2 * sigma^p with t = -1/sigma^2 * noise (dsm.py:20-30; the batch mean of :32 is the
 *                 caller's); aux (optional) = d mean-loss / d scores = (s - t) * sigma^p / B.
 *   GRAD_ADD      out (+)= grad, or grad * ELU'(in) with SBC_PRO_ELU (in = the tensor the forward ELU was applied to).
 *   INORM_BWD     reverse of stats -> affine -> ELU: in = x, stats [B][3][cin] (forward), weight = alpha|gamma|beta,
 *                 grad = d / d ELU-output (or d / d norm-output without SBC_PRO_ELU); out (+)= d / d x through the
 *                 normalised value, the spatial mean / variance and the cross-channel mean term; wgrad = d alpha|gamma|beta
 *                 [3][cin] summed over the batch (written); aux = scratch, >= B*6*cin floats.
 *   MAXPOOL5_BWD  in = forward input, grad = d / d output; out (+)= the gradient routed to each window's first maximum in
 *                 row-major order (times ELU'(in) with SBC_PRO_ELU); aux = scratch, >= B*H*W*cin bytes.
 *   UPSAMPLE_BWD  grad = [B][H][W][cin]; out (+)= [B][up_h][up_w][cin], the transpose of the resize of SBC_EPI_UP.
 *   POOL_BWD      grad = [B][H/2][W/2][cin]; out = [B][H][W][cin] = grad[h/2][w/2] / 4.
 *   CONV_WGRAD    in/stats/flags(PRO_*)/ksize/dil as in the forward CONV, grad = d / d (conv + bias) [B][H][W][cout];
 *                 wgrad = [cout][cin][k][k] (torch layout, written), bgrad = [cout] or NULL; aux = scratch (float),
 *                 >= sbc_wgrad_scratch_floats(B, H, W, cin, cout, ksize) (one buffer serves all launches of a stream).
 *   PACK_WEIGHT   in = [cout][cin][k][k] float32 DEVICE, out = the sbc_pack_conv_weight_split layout (of the adjoint
 *                 convolution cout -> cin with SBC_PACK_ADJOINT).  Batched form (aux != NULL): aux = device int32 table
 *                 [B][6] = (source offset from `in` in floats, destination offset from `out` in uint16, cout, cin, k*k
 *                 or 16 for the Winograd form, adjoint) and cin/cout = those of the largest entry: every weight of a
 *                 network in one launch.
 *   END_CONV_BWD  in/stats/weight/ext as in END_CONV, grad = d / d score [B][H][W][2]; out = d / d ELU-output
 *                 [B][H][W][cin] (written); wgrad [2][cin][3][3], bgrad [2]; aux = scratch >= sbc_wgrad_scratch_floats.
 *   BEGIN_CONV_BWD in = x [B][H][W][2], grad = d / d output [B][H][W][cout]; wgrad [cout][2][3][3], bgrad [cout]; aux.
 *   ADAM_EMA      ext = sbc_adam; in = gradients [n], out = parameters [n] (updated in place), aux = state [3][n]:
 *                 exp_avg | exp_avg_sq | EMA shadow.
 */
typedef struct sbc_dsm {
    const float* sigmas;         /* [num_classes] device */
    const int64_t* labels;       /* [B] device: noise level of each sample (dsm.py:9-12) */
    const float* noise;          /* [B][n] device standard-normal draws to replay, or NULL -> Philox */
    const int64_t* sample_id;    /* [B] device Philox stream ids or NULL (= b) */
    uint64_t seed;
    int32_t offset;              /* Philox counter word 1 (the optimiser step) = offset + *step */
    float anneal_power;          /* dsm.py:7 (2 in train_score.py:55) */
    const int32_t* step;         /* device step counter or NULL (= 0): lets a replayed plan draw fresh noise every step */
    float grad_scale;            /* DSM_LOSS: extra factor on d loss / d scores; 0 means 1.  1 / world_size makes the SUM
                                    all-reduce of data-parallel ranks the gradient of the mean over the global batch */
} sbc_dsm;

typedef struct sbc_adam {
    int64_t n;                   /* elements */
    double lr, beta1, beta2, eps; /* torch.optim.Adam(lr, betas, eps), weight_decay = 0, amsgrad = False.  double: torch
                                    forms 1 - beta and the bias corrections from python floats before rounding to fp32 */
    double ema_mu;               /* EMAHelper(mu): shadow = (1 - mu) * p + mu * shadow; < 0 disables the shadow update */
    const int32_t* step;         /* device counter: number of optimiser steps already taken (t - 1) */
} sbc_adam;

/* Extension of SBC_OP_CHAIN: the blocks, in execution order.  Every convolution is 3x3, cin = cout = op.cin:
 *   SBC_CHAIN_RCU   x <- x + conv_w2(ELU(conv_w1(ELU(x))))                      (no bias)                 layers.py:126-134
 *   SBC_CHAIN_CRP   x <- ELU(x); p = conv_w1(maxpool5(x)); x <- p + x; q = conv_w2(maxpool5(p)); x <- q + x   (no bias)   layers.py:76-83
 *   SBC_CHAIN_RES   a ResidualBlock without resampling or channel change (layers.py:443-456, normalization.py:163-176):
 *                   x <- shortcut + conv_w2(ELU(norm2(conv_w1(ELU(norm1(x))) + bias1))) + bias2, every convolution with dilation
 *                   dil (1, or 2 / 4 at a width of two); shortcut = x, or conv_w3(x) + bias3 when w3 is set (the dilated 'down'
 *                   blocks); norm1 / norm2 = alpha | gamma | beta [3][cin] of the two InstanceNorm++ layers: the launch forms their
 *                   statistics itself, a workgroup holds whole samples
 * w1 / w2 / w3: sbc_pack_conv_weight_f16x2 forms (SBC_CONV_F16X2 must be set: the only multiplier the kernel has).  w1_wino / w2_wino:
 * the same layers' sbc_pack_conv_weight_winograd_f16x2 forms or NULL -- never read by a kernel, but sbc_f16x2_calibrate writes the
 * layer's activation scale into every form it is handed (see sbc_op.weight2_wino_split). */
#define SBC_CHAIN_MAX_BLOCKS 6
#define SBC_CHAIN_RCU 0
#define SBC_CHAIN_CRP 1
#define SBC_CHAIN_RES 2
typedef struct sbc_chain {
    int32_t n_blocks;
    int32_t type[SBC_CHAIN_MAX_BLOCKS];
    int32_t dil[SBC_CHAIN_MAX_BLOCKS];             /* RES blocks; 0 or 1 = undilated */
    const void* w1[SBC_CHAIN_MAX_BLOCKS];
    const void* w2[SBC_CHAIN_MAX_BLOCKS];
    const void* w1_wino[SBC_CHAIN_MAX_BLOCKS];
    const void* w2_wino[SBC_CHAIN_MAX_BLOCKS];
    const void* w3[SBC_CHAIN_MAX_BLOCKS];          /* RES: shortcut convolution or NULL */
    const float* bias1[SBC_CHAIN_MAX_BLOCKS];      /* RES */
    const float* bias2[SBC_CHAIN_MAX_BLOCKS];
    const float* bias3[SBC_CHAIN_MAX_BLOCKS];
    const float* norm1[SBC_CHAIN_MAX_BLOCKS];
    const float* norm2[SBC_CHAIN_MAX_BLOCKS];
} sbc_chain;

/* Extension of SBC_OP_END_CONV: where the noise level comes from (ncsnv2.py:295-298). */
typedef struct sbc_endconv {
    const float* sigmas;         /* [num_classes] device, float32 (models/__init__.py:4-8) */
    const int64_t* labels;       /* [B] device or NULL */
    const float* sigma_of_step;  /* [n_steps] device: sigma of the level walked at step k (if labels NULL) */
    const int32_t* step;         /* device step counter */
} sbc_endconv;

/* Extension of SBC_OP_LANGEVIN and SBC_OP_MEASURE.  All complex tensors are interleaved float32 pairs.
 *   X      [B][Nt][Nr]  current estimate, updated in place            (test_score.py:164-165)
 *   score  [B][Nt][Nr]  output of the score plan                       (:150-154)
 *   P      [nP][Np][Nt] conj-transposed pilots, sample b uses P[p_index[b]] (b if p_index NULL)   (:109-111)
 *   Y      [B][Np][Nr]  measurements                                   (:122-124)
 *   Htrue  [nH][Nt][Nr] ground truth, sample b uses Htrue[h_index[b]]  (:112-113,131)
 *   sched  [G][n_steps][4] float32 (alpha, dc_div, noise_scale, dc_boost) of group `group[b]` at step k,
 *          i.e. the float64 python scalars of :143-144,160,165 rounded to float32; dc_boost (1 for test_score,
 *          --dc_boost of test_mmse.py:231-233) multiplies the data-consistency gradient before the division; 0 means
 *          "not set" and is read as 1 (hosts written against the three-column table of ABI <= 4)
 *   noise  [n_steps][B][Nt][Nr] CN(0,1) draws or NULL -> in-kernel Philox4x32-10: elements 2q, 2q+1 of a trajectory share
 *          the block of counter (q, step, traj_id lo, traj_id hi), key = seed; words (x, y) / (z, w) feed one Box-Muller
 *          each (csrc/philox.h; restated on the host by oracle/ald_oracle.py::device_complex_normal)      (:160-161)
 *   nmse   [n_steps][B] float32 log, row *step is written               (:168-170)
 * SBC_OP_MEASURE reads Htrue and P and writes Y; its `noise` is [B][Np][Nr] and `meas_scale[b]` =
 * float32(sqrt(local_noise)).
 * Constraints of SBC_OP_LANGEVIN (checked, SBC_ERR_INVALID otherwise): Nr is EVEN -- the update takes the elements of a row in
 * adjacent pairs (one Philox block, one pilot value, 16-byte accesses) -- and X, score, P, Y, Htrue and noise are 16-byte aligned
 * (Nt * Nr even keeps every per-trajectory slice aligned too; P is copied 16 bytes at a time where its rows are staged on chip).
 * Every refusal names the field; sbc_plan_create makes the same checks of LANGEVIN, MEASURE and STEP_INC records as sbc_op_launch.
 * The score network itself needs Nt, Nr multiples of 8.
 */
typedef struct sbc_langevin {
    float* X;
    const float* score;
    const float* P;
    const int32_t* p_index;
    float* Y;
    const float* Htrue;
    const int32_t* h_index;
    const float* sched;
    const int32_t* group;
    const float* noise;
    float* nmse;
    const int32_t* step;
    const int64_t* traj_id;
    const float* meas_scale;
    uint64_t seed;
    int32_t n_steps, Nt, Nr, Np;
} sbc_langevin;

typedef struct sbc_plan sbc_plan;

/* --- library ----------------------------------------------------------------------------------- */
int sbc_abi_version(void);
/* (ABI 12) The persistent kernels (SBC_OP_CONV_PAIR / CONV_POOL / RES_BLOCK and the direct kernel behind SBC_OP_CONV) size their grids for
 * `n` CUs instead of all of them; 0 = all (the default).  A host that keeps TWO independent launch streams busy sets half the device's
 * CUs, so that the two streams' persistent launches are resident side by side instead of one after the other (measured: -0.7 % per
 * two-stream Langevin step; results do not depend on it).  Process-wide DEFAULT; takes effect for launches issued after the call.
 * Prefer sbc_plan_set_persistent_cus (below): a plan's own width does not race with other threads, handles or devices. */
int sbc_set_persistent_cus(int32_t n);
const char* sbc_last_error(void);
/* number of visible HIP devices, or a negative sbc_status (does not initialise a device context) */
int sbc_device_count(void);

/* --- single operator (unit tests, ad-hoc use) ---------------------------------------------------- */
/* Launch one fused operator asynchronously on `stream` (a hipStream_t, may be NULL = default stream). */
int sbc_op_launch(const sbc_op* op, void* stream);

/* --- plans ---------------------------------------------------------------------------------------
 * sbc_plan_create copies `ops` (and their `ext` structs); the device buffers they point to must outlive the
 * plan.  sbc_plan_run executes the whole op list `n_iters` times in order on `stream` -- records with a `lane` (ABI 14) on the
 * library's lane streams: every lane is forked from `stream` at the start of the call and joined into it at its end (not between
 * the iterations, where the records' own events order the lanes), so that a caller sees ONE asynchronous unit of work.  With
 * use_graph = 1 and lanes the captured graph is flat (lane records on the run stream in list order); use_graph = 2 keeps the lanes as
 * parallel branches of the graph (experimental: the runtime's graph launch is not robust with them, see csrc/api.hip).  With
 * use_graph != 0 the op list is captured once into a hipGraph (on first use for that stream) and replayed;
 * this is legal because nothing in a plan depends on host state -- step-dependent scalars are read from
 * device tables through the device step counter. */
int sbc_plan_create(const sbc_op* ops, int32_t n_ops, sbc_plan** out_plan);
int sbc_plan_run(sbc_plan* plan, void* stream, int32_t n_iters, int32_t use_graph);
/* (ABI 13) Grid width, in CUs, of the persistent kernels of THIS plan's launches (0 = the process default above).  The setting is a
 * field of the plan, applied on the calling host thread for the duration of sbc_plan_run (and baked into a captured graph; changing
 * it drops the captured graph): plans driven from different host threads, for different streams or devices, are independent of each
 * other -- the library holds no mutable state shared between handles on this path.  Results never depend on it. */
int sbc_plan_set_persistent_cus(sbc_plan* plan, int32_t n);
void sbc_plan_destroy(sbc_plan* plan);

/* Per-kernel timing for the roofline report: while enabled (tag >= 0), every launch of an op whose
 * `tag` matches is bracketed by a hipEvent pair on the launch stream (eager runs only).  sbc_plan_profile_read
 * synchronises on the recorded events, returns the summed kernel time and launch count since enabling, and
 * resets the accumulators. */
int sbc_plan_profile(sbc_plan* plan, int32_t tag);
int sbc_plan_profile_read(sbc_plan* plan, double* total_ms, int64_t* n_launches);

/* --- helpers --------------------------------------------------------------------------------------
 * Host-side re-ordering of a torch-layout convolution weight [cout][cin][k][k] into the MFMA B-operand
 * fragment order consumed by SBC_OP_CONV: [k*k][cin/8][cout/32][64 lanes][4].  dst and src are HOST
 * pointers; cin % 8 == 0, cout % 32 == 0. */
int sbc_pack_conv_weight(const float* src, int32_t cout, int32_t cin, int32_t ksize, float* dst);
/* Same for the Winograd form of a 3x3 weight: U = G g G^T per (cout, cin) (computed in double), packed with the 16
 * transform positions in place of the taps: [16][cin/8][cout/32][64][4]. */
int sbc_pack_conv_weight_winograd(const float* src, int32_t cout, int32_t cin, float* dst);
/* Split-bf16 form: w = wh + wm + wl with wh = bf16(w), wm = bf16(w - wh), wl = bf16(w - wh - wm) (round to nearest
 * even; the sum is exact), as bf16 bit patterns in B-operand fragment order [k*k][cin/16][cout/32][3][64 lanes][8]:
 * lane l of block (tap, g, n) holds w[n*32 + (l & 31)][g*16 + 8*(l >> 5) + j][tap], j = 0..7.  cin % 16 == 0. */
int sbc_pack_conv_weight_split(const float* src, int32_t cout, int32_t cin, int32_t ksize, uint16_t* dst);
/* Winograd form U = G g G^T (double, rounded once to float) of a 3x3 weight, split like sbc_pack_conv_weight_split with
 * the 16 transform positions in place of the taps: [16][cin/16][cout/32][3][64][8] uint16. */
int sbc_pack_conv_weight_winograd_split(const float* src, int32_t cout, int32_t cin, uint16_t* dst);

/* --- the whole score network behind one call (hosts that are not Python) -------------------------------
 * NCSNv2Deepest.forward (ncsnv2/models/ncsnv2.py:269-300) becomes ~150 sbc_op records: the library wires them and shares
 * activation storage between them and turns them into sbc_op records over a host's memory (sbc_score_wiring_* below: one wiring, one
 * binder); a host packs the weights, allocates device memory and says where each packed form lives (the Python host:
 * score_based_channels_amd/scorenet.py).  sbc_score_create does all of that inside the library from the tensors of the reference checkpoint's
 * `model_state` (names as in NCSNv2Deepest.state_dict(): "res2.0.conv2.conv.weight", "normalizer.alpha", ...; HOST
 * pointers, float32, torch layouts).  The handle owns its device memory (weights, activation slots for `batch` samples,
 * labels).  conv_mode: 0 = split-bf16 (fp32-accurate), 1 = fp32 MFMA, 2 = fp16 weights (SBC_CONV_F16W; every parameter is
 * rounded to fp16 first), 3 = f16x2 (SBC_CONV_F16X2: fp32-class on the fp16 matrix cores, default of the Python host).
 *   sbc_score_buffers      device pointers of the input x [batch][Nt][Nr][2], the output score (same shape) and the
 *                          int64 noise-level labels [batch] (ncsnv2.py:295-298); fill x / labels, then
 *   sbc_score_forward      one score evaluation, asynchronous on `stream`;
 *   sbc_score_level_source inside an annealed-Langevin plan: take sigma from sigma_of_step[*step] (device) instead of
 *                          the labels (both NULL switches back);
 *   sbc_score_ops          the bound records, e.g. to append SBC_OP_LANGEVIN + SBC_OP_STEP_INC (X = the x buffer,
 *                          score = the out buffer) and build a full Langevin-step plan with sbc_plan_create. */
typedef struct sbc_tensor_ref { const char* name; const float* data; int64_t numel; } sbc_tensor_ref;
typedef struct sbc_score_desc {
    int32_t ngf, channels;       /* 32, 2 (train_score.py:37,59) */
    int32_t nt, nr;              /* array size; multiples of 8 */
    int32_t batch;
    int32_t conv_mode;
    const float* sigmas;         /* HOST [num_classes] (models/__init__.py:4-8) */
    int32_t num_classes;
    int32_t flags;               /* ABI 9: SBC_SCORE_* */
} sbc_score_desc;
#define SBC_SCORE_FOLD_STATS 0x2 /* InstanceNorm++ statistics of the full-resolution tensors from the tile moments their producers write
                                    (SBC_EPI_MOMENTS_OUT / SBC_PRO_NORM_MOMENTS; not conv_mode 1; scorenet.DEFAULT_FOLD_STATS) */
#define SBC_SCORE_FUSE_PAIRS 0x1 /* every RCU block of 32 channels at a width of 16 as one SBC_OP_CONV_PAIR record, and (ABI 11) every CRP
                                    stage of that shape as one SBC_OP_CONV_POOL record (conv_mode 2 / 3); what the Python host does
                                    by default in those modes (scorenet.DEFAULT_FUSE_PAIRS) */
#define SBC_SCORE_FUSE_RES   0x4 /* (ABI 12) the ResidualBlocks without resampling at 64 x 16 as one SBC_OP_RES_BLOCK record each (conv_mode 3);
                                    what the Python host does by default next to SBC_SCORE_FUSE_PAIRS (scorenet.DEFAULT_FUSE_RES) */
#define SBC_SCORE_FUSE_CHAIN 0x8 /* (ABI 13) the RCU / CRP runs of the 8 x 2 level as SBC_OP_CHAIN records (conv_mode 3); what the Python host does by
                                    default next to SBC_SCORE_FUSE_PAIRS (scorenet.DEFAULT_FUSE_CHAIN) */
#define SBC_SCORE_FUSE_DOWN 0x10 /* (ABI 13) pooled conv2 + pooled 1x1 shortcut of the downsampling ResidualBlocks res2.0 / res3.0 as one SBC_OP_CONV_DOWN
                                    record (conv_mode 3); what the Python host does by default (scorenet.DEFAULT_FUSE_DOWN) */
#define SBC_SCORE_FUSE_END  0x20 /* (ABI 13) the normalizer's statistics inside the SBC_OP_END_CONV launch (SBC_PRO_NORM_SELF on that record: 32 channels,
                                    1024 pixels; any conv_mode); what the Python host does by default next to SBC_SCORE_FUSE_PAIRS
                                    (scorenet.DEFAULT_FUSE_END) */
#define SBC_SCORE_SKIP_LANES 0x40 /* (ABI 14) the decoder's skip branches (refineK.adapt_convs.0) behind their anchor records on launch lane 1 (sbc_op.lane /
                                    signal / wait): for small batches, where the low-resolution launches are latency-bound -- what the Python host does for
                                    batches of at most scorenet.SKIP_OVERLAP_MAX_T trajectories (identical results) */
typedef struct sbc_score sbc_score;
int sbc_score_create(const sbc_score_desc* desc, const sbc_tensor_ref* tensors, int32_t n_tensors, sbc_score** out);
int sbc_score_buffers(sbc_score* score, float** x, float** out, int64_t** labels);
int sbc_score_ops(sbc_score* score, const sbc_op** ops, int32_t* n_ops);
int sbc_score_level_source(sbc_score* score, const float* sigma_of_step, const int32_t* step);
int sbc_score_forward(sbc_score* score, void* stream);
void sbc_score_destroy(sbc_score* score);

/* --- the wiring of the score network and its binding to a host's memory, without a device (ABI 15, 16) ----------------
 * Which records one score evaluation consists of, in which order and on which launch lane, which logical tensors share a buffer, and
 * which packed form of which parameter each sbc_op field points at: what sbc_score_create runs, for hosts that own their device memory
 * (score_based_channels_amd/plan.py reads the wiring into its dataclasses, scorenet.py binds it).  Pure host code: none of the calls
 * initialises HIP or dereferences a pointer it binds.
 *   sbc_score_wiring_create   wires what `desc` asks for; with desc.conv_mode 0 .. 3 it first applies that mode's gates (below), with -1
 *                             none.  Refusals (SBC_ERR_INVALID, sbc_last_error):
 *                             Nt or Nr no multiple of 8, SBC_SCORE_SKIP_LANES with SBC_WIRING_OVERLAP, a skip branch that is not one
 *                             contiguous run of records or reads what its anchor does not have yet, a missing anchor, a lane outside
 *                             1 .. SBC_MAX_LANES-1, a third wait on one record, more than SBC_MAX_EVENTS events;
 *   sbc_score_wiring_read     flat arrays owned by the handle (strings included), valid until sbc_score_wiring_destroy;
 *   sbc_score_wiring_bind     (ABI 16) the wiring's records as sbc_op records over the caller's buffers -- the one place that knows which
 *                             form goes into which field, which SBC_CONV_* / SBC_PRO_ELU_ACC bits a conv_mode adds and how an sbc_chain
 *                             is filled. */
typedef struct sbc_skip_branch {
    const char* branch;          /* the contiguous run of records whose names start with this prefix ... */
    const char* anchor;          /* ... is issued behind the last record in front of it whose name starts with this one ... */
    int32_t lane;                /* ... on this launch lane, 1 .. SBC_MAX_LANES-1 (a branch no record matches is skipped) */
} sbc_skip_branch;
typedef struct sbc_score_wiring_desc {
    int32_t ngf, channels, nt, nr;
    int32_t flags;               /* SBC_SCORE_* | SBC_WIRING_* */
    const int32_t* pair_shapes;  /* SBC_SCORE_FUSE_PAIRS: n_pair_shapes x (channels, width) of the RCU blocks that become SBC_OP_CONV_PAIR records;
                                    NULL: (32, 16), or with conv_mode 2 that mode's longer list */
    int32_t n_pair_shapes;
    const sbc_skip_branch* skip; /* SBC_SCORE_SKIP_LANES: n_skip branches, hoisted in this order; NULL: the decoder's five skip branches on lane 1 */
    int32_t n_skip;
    int32_t conv_mode;           /* (ABI 16) -1: wire exactly what `flags` asks for.  0 bf16x3, 1 f32, 2 f16w, 3 f16x2: the records are for that
                                    multiplier -- SBC_SCORE_FOLD_STATS is dropped in mode 1 and for Nt or Nr that are no powers of two (the tile
                                    moments are written by the Winograd split kernels, which take power-of-two images), and mode 2 has its
                                    own default pair_shapes.  Which SBC_SCORE_FUSE_* a mode can run at all stays the host's business */
} sbc_score_wiring_desc;
#define SBC_WIRING_OVERLAP       0x100 /* independent branches below full resolution as SBC_OP_SIDE records, joined by an SBC_OP_JOIN record */
#define SBC_WIRING_PRIVATE_SLOTS 0x200 /* every tensor in a buffer of its own (training reads every activation again on the way back) */
typedef struct sbc_wiring_tensor { const char* name; int32_t h, w, c, slot; } sbc_wiring_tensor;     /* per sample, NHWC; slot: index into slot_elems
                                                                                                        (-1: named by no record -- a merged SBC_OP_CHAIN keeps it on chip) */
typedef struct sbc_wiring_block {                  /* one block of an SBC_OP_CHAIN record: state_dict keys, NULL = none */
    int32_t type, dil;                             /* SBC_CHAIN_*; dil: RES blocks */
    const char *w1, *w2, *bias1, *bias2, *norm1, *norm2, *w3, *bias3;      /* bias1 .. bias3: RES blocks only (w3 / bias3: its shortcut convolution) */
} sbc_wiring_block;
typedef struct sbc_wiring_record {
    int32_t kind, flags, ksize, dil, tag;          /* as in sbc_op (flags without SBC_OP_SIDE / SBC_OP_JOIN and without a conv_mode's SBC_CONV_* bits) */
    int32_t src, dst, stats, res1, res2, up;       /* indices into tensors, -1 = none */
    int32_t moments;                               /* second output: tile moments of dst (SBC_EPI_MOMENTS_OUT) */
    int32_t geom;                                  /* SBC_OP_INORM_STATS from tile moments: the tensor whose (H, W, C) the launch describes */
    int32_t side, join;                            /* SBC_WIRING_OVERLAP: the record takes SBC_OP_SIDE / SBC_OP_JOIN */
    int32_t lane, signal, wait[2];                 /* as in sbc_op */
    int32_t first_block, n_blocks;                 /* SBC_OP_CHAIN: blocks[first_block .. first_block + n_blocks) */
    const char* name;                              /* of the layer the record computes (skip branches and anchors are named by prefixes of it) */
    const char *weight, *bias, *weight2, *bias2;   /* state_dict keys, NULL = none; SBC_OP_INORM_STATS: weight = the norm's prefix */
    const char *norm2;                             /* SBC_OP_RES_BLOCK: the second norm's prefix */
    const char *norm_key;                          /* SBC_PRO_NORM_SELF: the prefix of the norm whose (alpha | gamma | beta) sbc_op.stats points at */
} sbc_wiring_record;
typedef struct sbc_score_wiring_view {
    const sbc_wiring_tensor* tensors;
    const sbc_wiring_record* records;
    const sbc_wiring_block* blocks;
    const int64_t* slot_elems;                     /* per-sample float32 elements of each buffer */
    int32_t n_tensors, n_records, n_blocks, n_slots;
    int32_t x, out;                                /* the network's input and output tensors, [nt][nr][channels] */
    int32_t n_chains;                              /* (ABI 16) the SBC_OP_CHAIN records among `records`: the sbc_chain structs a binding needs */
} sbc_score_wiring_view;
typedef struct sbc_score_wiring sbc_score_wiring;
int sbc_score_wiring_create(const sbc_score_wiring_desc* desc, sbc_score_wiring** out);
int sbc_score_wiring_read(const sbc_score_wiring* wiring, sbc_score_wiring_view* view);
void sbc_score_wiring_destroy(sbc_score_wiring* wiring);
/* Binding.  `params` says what the host packed and where it lives, by name: "<state_dict key>" (fp32: biases, the begin / end
 * convolutions, and in conv_mode 1 sbc_pack_conv_weight), "<key>#winograd" (mode 1), "<key>#split" (the mode's direct form),
 * "<key>#winograd_split" (its Winograd form), "<key>#pool" (sbc_pack_conv_weight_pooled_f16x2), and a norm's prefix for its
 * alpha | gamma | beta [3][C].  A form that a record's kernel reads and `params` lacks is refused (SBC_ERR_INVALID; the message names
 * the record and the form).  The forms that ride along only for sbc_f16x2_calibrate (see sbc_op.weight2_wino_split) -- the Winograd
 * forms of CONV_PAIR / CONV_POOL / RES_BLOCK layers and of the undilated layers of a CHAIN, and in `weight`, `weight_wino_split`,
 * `weight_wino` of a CONV_DOWN record the "#split" and "#winograd_split" forms of its first and the "#split" form of its second layer --
 * are bound in conv_mode 3 where `params` has them and are NULL otherwise: a host that shares one weight buffer between array sizes
 * packs them, a host with one size does not need to.  ops [n_records] and chains [n_chains] are the caller's; a CHAIN record's ext
 * points into `chains`, the END_CONV record's at `endconv`. */
typedef struct sbc_named_ptr { const char* name; const void* ptr; } sbc_named_ptr;
typedef struct sbc_score_bind_desc {
    int32_t batch, conv_mode;    /* sbc_op.B; 0 bf16x3, 1 f32, 2 f16w, 3 f16x2 */
    void* const* slots;          /* one device buffer per slot of the wiring, [batch * slot_elems[i]] floats */
    int32_t n_slots;
    const sbc_named_ptr* params;
    int32_t n_params;
    const sbc_endconv* endconv;  /* caller-owned, read at sbc_plan_create / sbc_op_launch like every ext */
} sbc_score_bind_desc;
int sbc_score_wiring_bind(const sbc_score_wiring* wiring, const sbc_score_bind_desc* desc, sbc_op* ops, sbc_chain* chains);

/* fp16 weight forms for SBC_CONV_F16W (round to nearest even): the layouts of sbc_pack_conv_weight_split /
 * sbc_pack_conv_weight_winograd_split with a single fp16 term, [k*k | 16][cin/16][cout/32][64 lanes][8] uint16.  The
 * Winograd form rounds U = G g G^T (double) once to fp16. */
int sbc_pack_conv_weight_f16(const float* src, int32_t cout, int32_t cin, int32_t ksize, uint16_t* dst);
int sbc_pack_conv_weight_winograd_f16(const float* src, int32_t cout, int32_t cin, uint16_t* dst);

/* f16x2 weight forms for SBC_CONV_F16X2: every weight (or Winograd-transformed weight U = G g G^T, double -> float) is
 * scaled by 2^s -- s chosen per layer so that the largest magnitude lies in [2^13, 2^14) -- and written as two fp16 terms
 * h = fp16(w 2^s), l = fp16(w 2^s - h), in the layout of sbc_pack_conv_weight_split with 2 terms,
 * [k*k | 16][cin/16][cout/32][2][64 lanes][8] uint16, followed by a 16-byte trailer of four float32: (act_scale = 1, descale =
 * 1 / (act_scale 2^s), 2^-s, 0); act_scale must be a power of two (sbc_f16x2_calibrate sets it per layer on the device copy; a
 * host that knows its activations may write the first two words itself).  dst holds sbc_f16x2_elems(...) uint16. */
#define SBC_F16X2_ACT_SHIFT 0
#define sbc_f16x2_elems(taps, cin, cout) ((size_t)(taps) * (cin) * (cout) * 2 + 8)
/* (ABI 13) The filter of `meanpool2(conv(x))` as ONE stride-2 convolution, in the sbc_pack_conv_weight_f16x2 form with ksize + 1 taps per side:
 * src [cout][cin][ksize][ksize] (ksize 3 -> a 4x4 filter, ksize 1 -> 2x2), W'[p][q] = 1/4 sum_{a,b in {0,1}} W[p - a][q - b] formed in double.
 * dst: sbc_f16x2_elems((ksize + 1)^2, cin, cout) uint16. */
int sbc_pack_conv_weight_pooled_f16x2(const float* src, int32_t cout, int32_t cin, int32_t ksize, uint16_t* dst);
int sbc_pack_conv_weight_f16x2(const float* src, int32_t cout, int32_t cin, int32_t ksize, uint16_t* dst);
int sbc_pack_conv_weight_winograd_f16x2(const float* src, int32_t cout, int32_t cin, uint16_t* dst);
/* Range flag of the f16x2 kernels on the CURRENT device, a bit set collected since the last reset:
 *   bit 0 (SBC_RANGE_OVERFLOW)   a convolution staged an activation with |x| * act_scale >= 16000: its high fp16 term (or a
 *                                Winograd transform sum of four) may have overflowed;
 *   bit 1 (SBC_RANGE_UNDERFLOW)  a whole wavefront's share of an input tile (>= 8 pixels x every channel) was non-zero but below
 *                                2^-6 after scaling: the low fp16 terms of that region are denormal, the products there carry a
 *                                relative error above 2^-19 instead of 2^-22.
 * Either way the results of that run are not fp32-class: run the batch again in split-bf16 mode (conv_mode 0), which has fp32's
 * range -- the Python host does that by itself (driver.run_trajectories) and records it in the result file.  Synchronises with
 * the whole device (every stream).  reset != 0 clears the word. */
#define SBC_RANGE_OVERFLOW  1
#define SBC_RANGE_UNDERFLOW 2
#define SBC_RANGE_ELU       4   /* a fused RCU launch (SBC_OP_CONV_PAIR evaluates ELU as exp(x) - 1 only) ran on a layer whose calibrated
                                   inputs are below 2^-4, where that form no longer has fp32's relative accuracy */
int sbc_range_flag(int32_t* flag, int32_t reset);

/* Per-layer activation scales of conv_mode f16x2 (ABI 11).  A two-term fp16 split x s = h + l is fp32-class only while l stays a
 * normal fp16 number, i.e. for |x s| >= 2^-3; the packers write act_scale s = 1, which is right for O(1) activations only.
 * sbc_f16x2_calibrate runs the records `ops` ONCE on the first sample of their buffers (B = 1; the caller has put
 * sbc_f16x2_calibration_input there: a fixed CN(0,1)-like pattern, so the result depends on the checkpoint and the array size,
 * never on the data or the batch), collects max |x| of what every SBC_CONV_F16X2 convolution stages, and rewrites the 16-byte
 * trailers of their weight forms in DEVICE memory: act_scale = the power of two that puts that maximum into [2^8, 2^9) (31x
 * head room below the overflow guard, two-term precision for everything down to 2^-11 of the maximum), descale accordingly.
 * InstanceNorm++ makes the network's activations independent of the input's magnitude, so one calibration per checkpoint holds
 * for every noise level; data that leaves the window anyway raises sbc_range_flag.  Synchronises `stream`; must not run while
 * other launches use the same weights.  sbc_score_create (conv_mode 3) calls it; the Python host does on its first bind. */
int sbc_f16x2_calibration_input(float* x_host, int64_t n);
int sbc_f16x2_calibrate(const sbc_op* ops, int32_t n_ops, void* stream);

/* Known-answer hooks of the in-kernel random numbers (tests; synchronous, current device):
 *   sbc_debug_philox4x32     n blocks of Philox4x32-10 from host (c0, c1, c2, c3, k0, k1) records -> host (x, y, z, w) records:
 *                            the Random123 known-answer vectors must come back;
 *   sbc_debug_complex_normal the CN(0,1) draws (re, im interleaved) SBC_OP_LANGEVIN (step >= 0) / SBC_OP_MEASURE (step = -1) use
 *                            for elements 0 .. n_elem-1 of trajectory `traj` at `step` under `seed`. */
int sbc_debug_philox4x32(const uint32_t* counters_keys, int32_t n, uint32_t* out);
int sbc_debug_complex_normal(uint64_t seed, int64_t traj, int32_t step, int32_t n_elem, float* out);

/* scratch floats SBC_OP_CONV_WGRAD / END_CONV_BWD / BEGIN_CONV_BWD need in `aux` for this shape */
int64_t sbc_wgrad_scratch_floats(int32_t B, int32_t H, int32_t W, int32_t cin, int32_t cout, int32_t ksize);

/* --- classical baselines (Fig. 5c of the paper): Lasso / fsAD and ML ----------------------------------------------------------
 * Batched solvers of independent problems, one launch each, asynchronous on `stream`.  Complex data are interleaved float32
 * (re, im); pointers are device pointers.  A problem's arithmetic does not depend on its position in the batch or on B.
 *
 * sbc_l1_lifted_run: `steps` iterations of accelerated proximal gradient (sigpy.alg.GradientMethod, accelerate=True, proxg =
 * sigpy.prox.L1Reg(lambda)) on the lifted-DFT l1 problem of src/score_based_channels/test_l1Fourier_lifted.py:125-190, for every
 * problem b of the batch:
 *     Ld = conj(ifft(eye(Nt), n=L Nt, norm='ortho'))  [Nt][n1],  Rd = ifft(eye(Nr), n=L Nr, norm='ortho').T  [n2][Nr]   (:125-130)
 *     f(X) = 1/2 ||P Ld X Rd - Y||^2;  x = z = 0, t = 1;  per step  x_old = x;  x = soft(lambda lr, z - lr grad f(z));
 *     t' = (1 + sqrt(1 + 4 t^2)) / 2;  z = x + (t - 1) / t' (x - x_old);  t = t'                                       (:145-166)
 *     nmse[k][b] = ||Ld x Rd - H||^2 / ||H||^2 of the new x                                                              (:168-178)
 * soft(tau, v) = max(|v| - tau, 0) v / |v| (0 where v = 0).  Nothing is clamped: a step size above 1 / ||P||^2 diverges to
 * inf / NaN as the reference does.  Supported: Nt = 64, Nr = 16, 1 <= Np <= Nt, lifting L in {1, 2, 4} (n1 = L Nt, n2 = L Nr);
 * other shapes return SBC_ERR_UNSUPPORTED.  A p_index / h_index entry outside [0, nP) / [0, nH) gives a NaN log for that problem
 * and fills its H_hat and X (where given) with NaN; nothing is read through the bad index and no other problem is affected.
 * A refused call (any status but SBC_OK) has written nothing; B = 0 is SBC_OK and launches nothing. */
typedef struct sbc_l1_lifted_desc {
    const float* P;            /* [nP][Np][Nt] pilots, val_P of :112-113                                                       */
    const int32_t* p_index;    /* [B] pilot matrix of problem b, or NULL = b                                                   */
    const float* Y;            /* [B][Np][Nr] measurements, val_Y of :137-140                                                   */
    const float* Htrue;        /* [nH][Nt][Nr] channels, val_H of :114-115 (the NMSE reference)                                 */
    const int32_t* h_index;    /* [B] channel of problem b, or NULL = b                                                        */
    const float* lmbda;        /* [B] l1 weight (L1Reg lamda, :133)                                                             */
    const float* lr;           /* [B] step size (GradientMethod alpha, :159-161)                                                */
    float* nmse;               /* [steps][B] float32 per-step NMSE log (complete_log, :172-178)                                 */
    float* H_hat;              /* [B][Nt][Nr] final Ld x Rd (:181), or NULL                                                     */
    float* X;                  /* [B][n1][n2] final x (val_H_hat), or NULL                                                      */
    int32_t B, nP, nH, Nt, Nr, Np, lifting, steps;
} sbc_l1_lifted_desc;
int sbc_l1_lifted_run(const sbc_l1_lifted_desc* desc, void* stream);

/* sbc_ls_regularized: per problem b, H_hat = (P^H P + s2 I_Nt)^-1 P^H Y with s2 = noise_var[b] (src/score_based_channels/
 * test_ml.py:132-138, there 10^(-SNR/10), no Nt factor), solved as the equivalent system of size min(Np, Nt) -- for Np <= Nt
 * H_hat = P^H (P P^H + s2 I_Np)^-1 Y -- by an fp32 Cholesky factorisation; and nmse[b] = ||H_hat - H||^2 / ||H||^2 (:141-145).
 * noise_var must be > 0 (not checked on the device).  Supported: min(Np, Nt) <= 64, Nr <= 64, Nt, Np <= 1024; other shapes return
 * SBC_ERR_UNSUPPORTED.  A p_index entry outside [0, nP) -- or, with Htrue, an h_index entry outside [0, nH) -- fills that problem's
 * H_hat with NaN and gives a NaN nmse (where given); nothing is read through the bad index and no other problem is affected.
 * A refused call has written nothing; B = 0 is SBC_OK and launches nothing. */
typedef struct sbc_ls_desc {
    const float* P;            /* [nP][Np][Nt] pilots (val_P, :109-111)                                                        */
    const int32_t* p_index;    /* [B] or NULL = b                                                                              */
    const float* Y;            /* [B][Np][Nr] measurements (val_Y, :125-129)                                                    */
    const float* noise_var;    /* [B] s2 (local_noise, :135)                                                                   */
    const float* Htrue;        /* [nH][Nt][Nr] channels, or NULL (then nmse must be NULL)                                      */
    const int32_t* h_index;    /* [B] or NULL = b                                                                              */
    float* H_hat;              /* [B][Nt][Nr] estimate (est_H, :138)                                                           */
    float* nmse;               /* [B] or NULL (oracle_log, :141-145)                                                           */
    int32_t B, nP, nH, Nt, Nr, Np;
} sbc_ls_desc;
int sbc_ls_regularized(const sbc_ls_desc* desc, void* stream);

/* sbc_em_gm_amp_run: the EM-GM-AMP baseline of matlab/test_em_gm_amp.m, for every problem b of the batch, all iterations in one
 * launch (csrc/cs_gamp.hip).  THE LIMIT: the script only calls EMGMAMP(...) from a MATLAB toolbox that is not in the reference's
 * tree.  The toolbox's source is not available, so its internals -- adaptive step sizes, the order of its EM updates, its
 * initialisation -- are neither reproduced nor compared against.  Reproduced is the SCRIPT: its operator (:99-101), noise model
 * (:112-113), schedule (:58-59, :67), configuration and logs (:123-138).  The ALGORITHM is the one defined here, restated from the
 * published method (Bernoulli Gaussian-mixture GAMP with an EM-learned prior and noise variance); its yardstick is the float64
 * numpy restatement of this same definition, tests/gamp_oracle.py.
 *     unknown  X = fft2(H) (:99):  H = Fl X Fr,  Fl = conj(dftmtx(Nt)) / Nt,  Fr = conj(dftmtx(Nr)) / Nr (:37-38);  A1 = P Fl,
 *              Y = A1 X Fr + noise (:101);  a2 = |A1|^2,  M = Np Nr,  N = Nt Nr
 *     prior    p(x) = (1 - lam) delta(x) + lam sum_{l=1..4} om_l CN(x; 0, phi_l)  (optEM.heavy_tailed), noise variance psi; one
 *              parameter set per problem (sig_dim = noise_dim = 'col' on a single column)
 *     init     lam = Np / (2 Nt);  psi = ||Y||^2 / (101 M);  phibar = (||Y||^2 - M psi) / (||A1||_F^2 lam);  om_l = 1/4;
 *              phi_l = phibar 4^(l-1) 4/85;  xhat = 0;  taux = lam phibar;  s = 0
 *     one GAMP iteration (damping theta):
 *              taup[p] = (1 / Nr^2) sum_i a2[p][i] sum_j taux[i][j];   phat = A1 xhat Fr - taup s
 *              s_new = (Y - phat) / (taup + psi);  taus_new = 1 / (taup + psi);  zhat = phat + taup s_new;  tauz = taup psi / (taup + psi)
 *              s <- (1 - theta) s + theta s_new,  taus likewise (the very first iteration of a problem takes the new values undamped)
 *              taur[i] = Nr / sum_p a2[p][i] taus[p];   rhat = xhat + taur (A1^H s Fr^H)
 *              denoiser per coefficient, log domain, the largest of the five log-weights subtracted before exp:
 *                log a_0 = log(1 - lam) - log taur - |rhat|^2 / taur;   log a_l = log(lam om_l) - log(phi_l + taur) - |rhat|^2 / (phi_l + taur)
 *                beta = a / sum a;  g_l = phi_l / (phi_l + taur);  m_l = phi_l taur / (phi_l + taur) + g_l^2 |rhat|^2
 *                xhat = sum_l beta_l g_l rhat;   taux = sum_l beta_l m_l - |xhat|^2
 *     one EM iteration = nit GAMP iterations (xhat, taux, s, taus carry over), then from the last iteration's quantities, with
 *              pi = sum_{l>=1} beta_l:  lam <- clamp(mean pi, 1/N, 1);  om_l <- sum beta_l / sum pi;
 *              phi_l <- max(sum beta_l m_l / sum beta_l, 1e-12 phibar) (unchanged where sum beta_l = 0);
 *              psi <- mean over (p, r) of |Y - zhat|^2 + tauz;   nmse[k][b] = ||Fl xhat Fr - H||^2 / ||H||^2  (complete_log, :127-136)
 *     stop     with tol > 0 a problem stops after the first EM iteration with ||xhat - xhat_prev||^2 < tol ||xhat||^2 (xhat_prev:
 *              the end of the EM iteration before, 0 at the start); its remaining nmse rows hold the script's sentinel 1000 (:71),
 *              stop_iter[b] the number of EM iterations it ran.  tol = 0 never stops.
 * The whole iteration runs in float64 (products on v_mfma_f64_16x16x4_f64; the iteration is not contractive at fp32 resolution,
 * DESIGN.md section 18); operands and outputs are fp32, theta and tol are the fp32 values given.  Fixed summation orders, no
 * atomics: a problem's result is bit-identical whatever the batch and its position in it; NaN / Inf stay inside their problem.
 * Supported: Nt = 64, Nr = 16, 1 <= Np <= 64, nit >= 1, em_iters >= 1, 0 < theta <= 1; anything else returns SBC_ERR_UNSUPPORTED.
 * A p_index / h_index entry outside [0, nP) / [0, nH) fills that problem's outputs (where given; stop_iter: -1) with NaN; nothing
 * is read through the bad index and no other problem is affected.  A refused call (any status but SBC_OK) has written nothing;
 * B = 0 is SBC_OK and launches nothing.  The first call on a device allocates and uploads two small twiddle tables synchronously
 * (kept for the life of the process, as sbc_l1_lifted_run keeps its own): that one call is not asynchronous and cannot be captured. */
typedef struct sbc_em_gm_amp_desc {
    const float* P;            /* [nP][Np][Nt] pilots, local_P of :81                                                          */
    const int32_t* p_index;    /* [B] pilot matrix of problem b, or NULL = b                                                   */
    const float* Y;            /* [B][Np][Nr] noisy measurements, noisy_flat_Y of :112-113 as a matrix                          */
    const float* Htrue;        /* [nH][Nt][Nr] channels, local_H of :95, or NULL (then nmse must be NULL)                       */
    const int32_t* h_index;    /* [B] channel of problem b, or NULL = b                                                        */
    float* nmse;               /* [em_iters][B] NMSE after every EM iteration (complete_log), or NULL                           */
    float* H_hat;              /* [B][Nt][Nr] final Fl xhat Fr (:118-120), or NULL                                              */
    float* X;                  /* [B][Nt][Nr] final xhat, or NULL                                                              */
    float* params;             /* [B][10] final lam, om_1..4, phi_1..4, psi, or NULL                                            */
    int32_t* stop_iter;        /* [B] EM iterations run, or NULL                                                               */
    int32_t B, nP, nH, Nt, Nr, Np, nit, em_iters;
    float theta, tol;          /* damping (0.3); optEM.maxTol (1e-1, :59)                                                       */
} sbc_em_gm_amp_desc;
int sbc_em_gm_amp_run(const sbc_em_gm_amp_desc* desc, void* stream);

/* --- Learned D-AMP (the L-DAMP baseline of Fig. 5c) -----------------------------------------------------------------------------
 * src/score_based_channels/test_ldamp.py with aux_models.py:62-190 (LDAMP.forward) and aux_unet.py (FlippedNormUnet), in the
 * configuration train_ldamp.py:41-47 trains: backbone FlippedUNet, one net per unroll (shared_nets = False), chans 16, 3 pools,
 * Nt x Nr = 64 x 16 (csrc/ldamp.hip).  Per unroll u, with the denoiser D_u(x) = x - unnorm(U_u(norm(x))):
 *     r = h + (1 / eig1) P^H z;  h = D_u(r);  eps = max(1e-3 max|r|, 1e-5);  h' = D_u(r + eps d);
 *     div = (1 / eps) mean over the 2048 reals of d (h' - h);  z = Y - P h + z div            (h = 0, z = Y before the first unroll)
 * Exact fp32 arithmetic, fixed summation orders, no atomics: a sample's result does not depend on its position in the batch or on
 * B, bit for bit.  Nothing is clamped: a constant re or im plane of r has a zero standard deviation and gives inf / NaN, as in the
 * reference.  Complex data are interleaved float32 (re, im); all data pointers are DEVICE pointers except where noted.
 *
 *   sbc_ldamp_create            copies the weights of n_nets denoisers from HOST tensors named as in the reference's state_dict,
 *                               "update_nets.<u>.unet.<...>" (19 per net, torch layouts; every name and element count is checked), to the
 *                               current device.  Synchronises (hipMemcpy).  The handle is bound to that device.
 *   sbc_ldamp_workspace_floats  float32 elements of `workspace` a run of B samples and num_unrolls unrolls needs (sbc_ldamp_denoise of B
 *                               images: the same with num_unrolls = 0); -1 on a negative argument.
 *   sbc_ldamp_denoise           out = D_net(r) for B images r [B][64][16][2]; asynchronous on `stream`.
 *   sbc_ldamp_run               num_unrolls (<= n_nets) unrolls for B samples; 19 launches per unroll (+ 1 for the directions, + 1 copy),
 *                               asynchronous on `stream`.  Every argument is checked before anything is launched; B = 0 launches nothing.
 *   sbc_ldamp_stage             where stage `stage` of the last call's images lies in its workspace: `offset` floats from the start, as
 *                               [n_images][channels][height][width] (n_images = B of sbc_ldamp_denoise, 2B of sbc_ldamp_run: image b is
 *                               the clean, B + b the perturbed evaluation of sample b in the last unroll).  Stages, in order: 0 r (complex
 *                               [64][16][2]), 1 norm(r), 2/3 first down block (conv 1, conv 2), 4 its pool, 5/6/7 second, 8/9/10 third, 11/12
 *                               bottleneck, then per up level (transposed conv, conv 1, conv 2): 13/14/15, 16/17/18, 19/20/21, and 22 the
 *                               norm's (mean_re, std_re, mean_im, std_im).  No stage shares memory with another.
 *   sbc_debug_ldamp_directions  (synchronous, current device) the direction d [64][16][2] -> HOST that a run without caller directions
 *                               uses for global sample id `sample` at `unroll` under `seed`: element (t, r) is the pair of N(0,1) draws
 *                               of one Philox4x32-10 block, counter (t * 16 + r, unroll, sample_lo, sample_hi), key = seed, Box-Muller on
 *                               words (x, y).  Written by the same kernel a run launches. */
typedef struct sbc_ldamp sbc_ldamp;
typedef struct sbc_ldamp_run_desc {
    const float* Y_herm;       /* [B][Np][16] complex measurements (sample['Y_herm'])                                            */
    const float* P_herm;       /* [B][Np][64] complex pilots (sample['P_herm'])                                                  */
    const float* eig1;         /* [B] (sample['eig1'])                                                                           */
    const float* directions;   /* [num_unrolls][B][64][16][2] random directions, or NULL = drawn on the device from (seed, sample0 + b, u) */
    const float* Htrue;        /* [B][64][16] complex channels for the NMSE, or NULL                                             */
    float* H_hat;              /* [B][64][16] complex: the last unroll's h (also the running h between unrolls)                  */
    float* nmse;               /* [B] ||H_hat - Htrue||^2 / ||Htrue||^2, or NULL                                                 */
    float* h_log;              /* [num_unrolls][B][64][16] complex h after every unroll, or NULL                                 */
    float* z_log;              /* [num_unrolls][B][Np][16] complex z after every unroll, or NULL                                 */
    float* div_log;            /* [num_unrolls][B], or NULL                                                                      */
    float* eps_log;            /* [num_unrolls][B], or NULL                                                                      */
    float* workspace;          /* sbc_ldamp_workspace_floats(B, num_unrolls) floats                                              */
    uint64_t seed;             /* of the device-drawn directions                                                                 */
    int64_t sample0;           /* global id of sample 0 (sample b draws from stream sample0 + b)                                 */
    int32_t B, Np, Nt, Nr, num_unrolls;   /* Nt = 64, Nr = 16, 1 <= Np <= 64                                                      */
} sbc_ldamp_run_desc;
int sbc_ldamp_create(const sbc_tensor_ref* tensors, int32_t n_tensors, int32_t n_nets, sbc_ldamp** out);
void sbc_ldamp_destroy(sbc_ldamp* handle);
int64_t sbc_ldamp_workspace_floats(int32_t B, int32_t num_unrolls);
int sbc_ldamp_denoise(sbc_ldamp* handle, int32_t net, const float* r, float* out, int32_t B, float* workspace, void* stream);
int sbc_ldamp_run(sbc_ldamp* handle, const sbc_ldamp_run_desc* desc, void* stream);
int sbc_ldamp_stage(int32_t stage, int32_t n_images, int64_t* offset, int32_t* channels, int32_t* height, int32_t* width);
int sbc_debug_ldamp_directions(uint64_t seed, int64_t sample, int32_t unroll, float* out);

/* --- Learned D-AMP training ---------------------------------------------------------------------------------------------------------
 * src/score_based_channels/train_ldamp.py:107-141 for the configuration above (csrc/ldamp_train.hip): the unrolled forward with every
 * unroll's activations kept, loss = mean_b sum |h - H|^2 and the logged NMSE = mean_b (sum |h - H|^2 / sum |H|^2), the gradient of the loss
 * with respect to the 19 tensors of the num_unrolls denoisers that ran, and one step of torch.optim.Adam (betas 0.9 / 0.999, eps 1e-8, no
 * weight decay).  div and eps are constants of the gradient (aux_models.py:148-171 computes them under no_grad): only the clean
 * evaluation is differentiated.  The forward is the launches of sbc_ldamp_run, so h, z, div and eps of every unroll are its bits.  Exact
 * fp32, fixed summation orders, no atomics: the stage gradients of a sample do not depend on B or its position in the batch; a parameter
 * gradient sums (sample, pixel) pairs in a fixed order.  1 <= B <= 128; all data pointers are DEVICE pointers except where noted.
 *
 *   sbc_ldamp_trainer_create            as sbc_ldamp_create; exp_avg, exp_avg_sq and the step count start at 0.  Synchronises.
 *   sbc_ldamp_trainer_workspace_floats  float32 elements of `workspace` for a step of B samples and num_unrolls unrolls (own_directions != 0:
 *                                       with room for device-drawn directions); -1 on an argument out of range.  Every unroll keeps its
 *                                       2B evaluation images and B gradient images: about 1.9 MB per sample and unroll.
 *   sbc_ldamp_trainer_step              forward, loss, backward and, with step >= 1, the Adam update of nets 0 .. num_unrolls - 1 with learning
 *                                       rate lr and bias corrections of step `step` (the host counts steps and schedules lr); step = 0:
 *                                       gradients only.  Launches: 19 per unroll + 1 directions + 1 or 2 copies, 2 for the loss, 54 per unroll
 *                                       for the backward, 1 Adam.  Asynchronous on `stream`; every argument is checked before anything is
 *                                       launched; B = 0 launches nothing.
 *   sbc_ldamp_trainer_adam              the Adam update alone, on `grads` ([n_nets][net floats], tensors in state_dict order; NULL: the
 *                                       gradients of the last step), for the first n_nets nets.  Asynchronous on `stream`.
 *   sbc_ldamp_trainer_stage             where a quantity of the last step lies in its workspace, as [n_images][channels][height][width] at
 *                                       `offset` floats: kind FORWARD (a stage of sbc_ldamp_stage's list, of unroll `unroll`, 2B images), GRAD (the
 *                                       loss gradient with respect to that stage of the clean evaluation, B images; stage 0: dL/dr, stage 22:
 *                                       the finish's share of d/d(mean, std)), RSTD (1 / sqrt(var + eps) of a stage's InstanceNorm, [2B][C]), GH
 *                                       (dL/dh_u as it reaches unroll u, [B][2048]), GZ (dL/dz_u for the z that enters unroll u: the slot has B * 2048 floats per unroll, of which the
 *                                       first B * Np * 32 hold [B][Np][16][2]), DIV ([B]).
 *   sbc_ldamp_trainer_get_state /       copy one of: 0 parameters, 1 gradients of the last step, 2 exp_avg, 3 exp_avg_sq ([n_nets][net floats],
 *   sbc_ldamp_trainer_set_state         tensors in state_dict order, HOST memory) and the step count out of / into the handle.  Synchronise
 *                                       the device. */
enum { SBC_LDAMP_TRAIN_FORWARD = 0, SBC_LDAMP_TRAIN_GRAD = 1, SBC_LDAMP_TRAIN_RSTD = 2, SBC_LDAMP_TRAIN_GH = 3, SBC_LDAMP_TRAIN_GZ = 4,
       SBC_LDAMP_TRAIN_DIV = 5 };
typedef struct sbc_ldamp_trainer sbc_ldamp_trainer;
typedef struct sbc_ldamp_step_desc {
    const float* Y_herm;       /* [B][Np][16] complex                                                                            */
    const float* P_herm;       /* [B][Np][64] complex                                                                            */
    const float* eig1;         /* [B]                                                                                            */
    const float* directions;   /* [num_unrolls][B][64][16][2], or NULL = drawn on the device from (seed, sample0 + b, u)         */
    const float* Htrue;        /* [B][64][16] complex (sample['H_herm_cplx'])                                                    */
    float* loss;               /* [2]: loss, NMSE (linear)                                                                       */
    float* h_log;              /* [num_unrolls][B][64][16] complex, or NULL                                                      */
    float* z_log;              /* [num_unrolls][B][Np][16] complex, or NULL                                                      */
    float* div_log;            /* [num_unrolls][B], or NULL                                                                      */
    float* eps_log;            /* [num_unrolls][B], or NULL                                                                      */
    float* workspace;          /* sbc_ldamp_trainer_workspace_floats(B, num_unrolls, directions == NULL) floats                  */
    uint64_t seed;
    int64_t sample0;
    double lr;                 /* learning rate of this step                                                                     */
    int64_t step;              /* 1-based count of this Adam step; 0: no update                                                  */
    int32_t B, Np, Nt, Nr, num_unrolls;
} sbc_ldamp_step_desc;
int sbc_ldamp_trainer_create(const sbc_tensor_ref* tensors, int32_t n_tensors, int32_t n_nets, sbc_ldamp_trainer** out);
void sbc_ldamp_trainer_destroy(sbc_ldamp_trainer* handle);
int64_t sbc_ldamp_trainer_workspace_floats(int32_t B, int32_t num_unrolls, int32_t own_directions);
int sbc_ldamp_trainer_step(sbc_ldamp_trainer* handle, const sbc_ldamp_step_desc* desc, void* stream);
int sbc_ldamp_trainer_adam(sbc_ldamp_trainer* handle, const float* grads, int32_t n_nets, double lr, int64_t step, void* stream);
int sbc_ldamp_trainer_stage(int32_t kind, int32_t stage, int32_t unroll, int32_t B, int32_t num_unrolls, int64_t* offset, int32_t* n_images,
                            int32_t* channels, int32_t* height, int32_t* width);
int sbc_ldamp_trainer_get_state(sbc_ldamp_trainer* handle, int32_t what, float* out, int64_t* step);
int sbc_ldamp_trainer_set_state(sbc_ldamp_trainer* handle, int32_t what, const float* in, int64_t step);

/* --- WGAN latent optimisation (the WGAN baseline of Fig. 5c) ---------------------------------------------------------------------
 * src/score_based_channels/test_wgan.py:129-176 with the generator aux_gan.py:58-112 (DCGAN_G_Ours) in eval mode, isize = [16, 64]
 * (Nr, Nt), nz = 60, nc = 2, ngf = 128, L = 2 + n_extra hidden layers, n_extra = 0 .. 4 read from the tensor names (csrc/wgan.hip):
 *     dense Linear(60 -> 8192) viewed [128][4][16];  layers 1, 2: nearest x 2, Conv 5 x 5 128 -> 128 + bias, BatchNorm (running
 *     statistics, eps 1e-5), ReLU;  layers 3 .. L: Conv 3 x 3 128 -> 128 (no bias), BatchNorm, ReLU;  out: Conv 5 x 5 128 -> 2 + bias.
 * One step of sample b, with G = gen[0] + i gen[1] [16][64]:  meas = ||G P - Y||_F^2, reg = ||z||^2, loss = s_b (meas + lambda_b reg),
 * g = d loss / d z, then torch.optim.Adam's defaults (betas 0.9 / 0.999, eps 1e-8, bias correction) on z with step size lr_b.  The logs
 * of step k are taken at z_k, before the update.  Samples are independent: lambda, lr and s are per-sample arrays (the reference's
 * torch.mean over its batch is s_b = 1 / kept_samples), so all (lambda, lr, SNR) cells of one pilot count run as one batch.
 * Exact fp32 arithmetic, the 128 -> 128 convolutions on the fp32 matrix cores, fixed summation orders, no atomics: a sample's result does
 * not depend on its position in the batch, on B or on repetition, bit for bit.  Complex data are interleaved float32 (re, im); all
 * data pointers are DEVICE pointers except where noted.
 *
 *   sbc_wgan_create            copies the generator from HOST float tensors named as in the reference's state_dict ("dense.dense_input.*",
 *                              "conv.conv1.*", "conv.bn1.{weight,bias,running_mean,running_var}", .., "conv.extra_conv<i>.weight",
 *                              "conv.extra_bn<i>.*", "conv.conv_out.*": 16 + 5 n_extra tensors, torch layouts, num_batches_tracked left
 *                              out; every name and element count is checked) to the current device and packs the filters for both
 *                              directions.  Synchronises (hipMemcpy).  The handle is bound to that device.
 *   sbc_wgan_workspace_floats  float32 elements of `workspace` a call with B samples needs; -1 on a bad argument.
 *   sbc_wgan_generate          out [B][2][16][64] = G(z [B][60]); L + 2 launches + 1 copy, asynchronous on `stream`.
 *   sbc_wgan_run               n_steps steps for B samples, 2 L + 4 launches per step, asynchronous on `stream`.  Every argument is checked
 *                              before anything is launched; B = 0 or n_steps = 0 launches nothing.
 *   sbc_wgan_stage             where a stage of the last call lies in its workspace: `offset` floats from the start, as
 *                              [B][channels][height][width].  Stages: k = 0 .. L the activations (0: the dense output [128][4][16], k >= 1:
 *                              layer k after its ReLU); 16 gen [2][16][64]; 17 dG = d loss / d gen; 32 + k, k = 0 .. L, d loss / d
 *                              (activation k); 48 + k, k = 1 .. L, the ReLU sign mask of layer k as 32-bit words [128][height][W / 32]
 *                              (bit j of word q: pixel x = 32 q + j is positive).  Stages 17 and 32 + k hold the last step of a run; a
 *                              generate call writes 0 .. L, 16 and the masks.  No stage shares memory with another. */
typedef struct sbc_wgan sbc_wgan;
typedef struct sbc_wgan_run_desc {
    const float* Y;            /* [B][16][Np] complex measurements (val_Y)                                                       */
    const float* P;            /* [B][64][Np] complex pilots (val_P)                                                             */
    const float* H;            /* [B][16][64] complex channels for oracle_log, or NULL                                           */
    float* z;                  /* [B][60] latents, in and out                                                                    */
    float* m;                  /* [B][60] Adam's exp_avg, in and out (zeros before the first step)                               */
    float* v;                  /* [B][60] Adam's exp_avg_sq, in and out                                                          */
    const float* lr;           /* [B]                                                                                            */
    const float* l2_lam;       /* [B]                                                                                            */
    const float* loss_scale;   /* [B] s_b                                                                                        */
    float* oracle_log;         /* [n_steps][B] ||G - H||^2 / ||H||^2, or NULL (needs H)                                          */
    float* meas_log;           /* [n_steps][B], or NULL                                                                          */
    float* reg_log;            /* [n_steps][B], or NULL                                                                          */
    float* z_log;              /* [n_steps][B][60] z before each update, or NULL                                                 */
    float* g_log;              /* [n_steps][B][60] d loss / d z of each step, or NULL                                            */
    float* workspace;          /* sbc_wgan_workspace_floats(handle, B) floats                                                    */
    int32_t B, Np;             /* 1 <= Np <= 64                                                                                  */
    int32_t first_step;        /* Adam's t of the first step (1 for a fresh run; continue a run with 1 + the steps already taken) */
    int32_t n_steps;
} sbc_wgan_run_desc;
int sbc_wgan_create(const sbc_tensor_ref* tensors, int32_t n_tensors, sbc_wgan** out);
void sbc_wgan_destroy(sbc_wgan* handle);
int64_t sbc_wgan_workspace_floats(const sbc_wgan* handle, int32_t B);
int sbc_wgan_generate(sbc_wgan* handle, const float* z, float* out, int32_t B, float* workspace, void* stream);
int sbc_wgan_run(sbc_wgan* handle, const sbc_wgan_run_desc* desc, void* stream);
int sbc_wgan_stage(const sbc_wgan* handle, int32_t stage, int32_t B, int64_t* offset, int32_t* channels, int32_t* height, int32_t* width);

/* --- WGAN training ----------------------------------------------------------------------------------------------------------------
 * src/score_based_channels/train_wgan.py:123-184 on the generator above and the critic aux_gan.py:9-56 (DCGAN_D), both in TRAINING mode
 * (BatchNorm on batch statistics, running statistics updated with momentum 0.1 and the unbiased variance), isize = [16, 64], nz = 60,
 * nc = 2, ngf = 128, ndf = 64, the same n_extra = 0 .. 4 for both networks, read from the tensor names (csrc/wgan_train.hip):
 *     D  layer 0: Conv 4 x 4 / 2 2 -> 64, LeakyReLU 0.2;  layers 1 .. n_extra: Conv 3 x 3 64 -> 64, BatchNorm, LeakyReLU;  layer n_extra + 1:
 *        Conv 4 x 4 / 2 64 -> 128, BatchNorm, LeakyReLU;  layer M = n_extra + 2: Conv (4, 16) 128 -> 1;  mean over the batch.  No bias.
 *   critic iteration     every parameter of D clamped to [clamp_lower, clamp_upper]; errD_real = mean_b D(real), backward with + 1;
 *                        fake = G(noise), no gradient through G; errD_fake = mean_b D(fake), backward with - 1, the gradients accumulate;
 *                        RMSprop on D
 *   generator iteration  fake = G(noise); errG = mean_b D(fake) (D's running statistics still update, its parameters get no gradient);
 *                        backward with + 1 through D's input and G's parameters; RMSprop on G; the filters are repacked
 *   RMSprop              torch.optim.RMSprop's defaults (no momentum, not centred): sq = alpha sq + (1 - alpha) g^2,
 *                        p = p + (- lr g) / (sqrt(sq) + eps), every operation rounded to fp32
 * fp32 arithmetic; the generator's 128 -> 128 convolutions run on the fp32 matrix cores in all three directions, the critic on the vector
 * ALUs; every sum over the batch is taken in float64 in a fixed order; no atomics: a sequence of calls run twice gives the same bits.
 * All data pointers are DEVICE pointers except where noted.
 *
 *   sbc_wgan_trainer_create   copies both networks from HOST float tensors named as in the reference's state_dict()s (the generator's as
 *                             for sbc_wgan_create; the critic's "main.initial:2-64:conv.weight", "main.extra-layers-<t>:64:conv.weight",
 *                             "main.extra-layers-<t>:64:batchnorm.{weight,bias,running_mean,running_var}", "main.pyramid:64-128:conv.weight",
 *                             "main.pyramid:128:batchnorm.*", "main.final:128-1:conv.weight": 7 + 5 n_extra tensors; num_batches_tracked is
 *                             left out, the caller counts) to the current device; gradients and square averages start at zero.  Every name
 *                             and element count is checked.  Synchronises.
 *   sbc_wgan_trainer_workspace_floats   float32 elements of a workspace with a capacity of B_cap samples per batch; -1 on a bad argument.
 *   sbc_wgan_trainer_critic_step        one critic iteration on real [B_real][2][16][64] and noise [B_fake][60]; losses [2] = errD_real,
 *                                       errD_fake (or NULL).  Asynchronous on `stream`; every argument is checked before the first launch.
 *   sbc_wgan_trainer_generator_step     one generator iteration on noise [B][60]; loss [1] = errG (or NULL).
 *   sbc_wgan_trainer_stage    where a stage of the last call lies in its workspace: `offset` floats from the start; per_sample = 1:
 *                             [B][channels][height][width] of the batch that wrote it, 0: [channels].  stage = 256 net + 16 kind + layer; net 0
 *                             the generator (layer k = 0 .. L, 0 the dense output), 1 the critic's pass over real, 2 its pass over fake
 *                             (layer j = 0 .. M); kind 0 activation, 1 raw convolution output (+ bias), 2 pre-activation, 3 sign mask of the
 *                             pre-activation as 32-bit words [channels][height][ceil(width / 32)] (bit j of word q: pixel 32 q + j), 4 batch
 *                             mean, 5 biased batch variance, 6 d loss / d activation, 7 d loss / d raw; net 0: 128 gen, 129 d loss / d gen;
 *                             net 1, 2: 130 the mean critic output [1].  No stage shares memory with another.
 *   sbc_wgan_trainer_copy     tensor `name` of net 0 (generator) / 1 (critic) between the device and the HOST array: what = 0 its value (parameters
 *                             and running statistics), 1 its gradient, 2 its RMSprop square average.  Synchronises the device.
 *   sbc_wgan_wgrad128, sbc_wgan_bn_backward, sbc_wgan_rmsprop   single launches of the step on the caller's operands:
 *                             dW [128][128][ks][ks] = sum_{b,y,x} draw[b][co][y][x] in[b][ci][y + ky - p][x + kx - p] (in read through the
 *                             nearest x 2 map with up = 1; scratch of sbc_wgan_wgrad128_scratch_floats);  the BatchNorm backward of one layer
 *                             from d loss / d activation (scratch: 2 C floats; dweight = sum dy xhat, dbias = sum dy);  RMSprop (mode 1) or the
 *                             clamp (mode 0) on n elements. */
typedef struct sbc_wgan_trainer sbc_wgan_trainer;
typedef struct sbc_wgan_trainer_desc {
    double lr_d, lr_g;         /* 5e-5 in the reference                                                                          */
    double alpha, eps;         /* torch.optim.RMSprop's defaults: 0.99, 1e-8                                                     */
    double clamp_lower, clamp_upper;   /* -0.01, 0.01                                                                            */
} sbc_wgan_trainer_desc;
int sbc_wgan_trainer_create(const sbc_wgan_trainer_desc* desc, const sbc_tensor_ref* gen, int32_t n_gen, const sbc_tensor_ref* disc, int32_t n_disc,
                            sbc_wgan_trainer** out);
void sbc_wgan_trainer_destroy(sbc_wgan_trainer* handle);
int64_t sbc_wgan_trainer_workspace_floats(const sbc_wgan_trainer* handle, int32_t B_cap);
int sbc_wgan_trainer_critic_step(sbc_wgan_trainer* handle, const float* real, int32_t B_real, const float* noise, int32_t B_fake, float* losses,
                                 float* workspace, int32_t B_cap, void* stream);
int sbc_wgan_trainer_generator_step(sbc_wgan_trainer* handle, const float* noise, int32_t B, float* loss, float* workspace, int32_t B_cap, void* stream);
int sbc_wgan_trainer_stage(const sbc_wgan_trainer* handle, int32_t stage, int32_t B_cap, int64_t* offset, int32_t* channels, int32_t* height,
                           int32_t* width, int32_t* per_sample);
int sbc_wgan_trainer_copy(sbc_wgan_trainer* handle, int32_t net, int32_t what, const char* name, float* host, int64_t numel, int32_t to_device);
int64_t sbc_wgan_wgrad128_scratch_floats(int32_t B, int32_t H, int32_t W, int32_t ks);
int sbc_wgan_wgrad128(const float* draw, const float* in, float* dW, float* scratch, int32_t B, int32_t H, int32_t W, int32_t ks, int32_t up,
                      void* stream);
int sbc_wgan_bn_backward(const float* gact, const float* raw, const int32_t* mask, const float* mean, const float* var, const float* weight, float slope,
                         float* draw, float* dweight, float* dbias, float* scratch, int32_t B, int32_t C, int32_t H, int32_t W, void* stream);
int sbc_wgan_rmsprop(float* p, const float* g, float* sq, int64_t n, double lr, double alpha, double eps, double clamp_lower, double clamp_upper,
                     int32_t mode, void* stream);

/* ---- Coded link simulation (csrc/link.hip; link.py, test_end_to_end.py) ----------------------------------------------------
 * What a channel estimate is worth to a receiver (matlab/test_end_to_end.m, testPackets.m, ComputeLLRMIMO.m 'ml'): packets of one
 * quasi-cyclic LDPC codeword each, QPSK on S spatial streams, exhaustive ML soft demapping once with the ideal and once with the
 * estimated precoded channel, sum-product decoding, BER / BLER per packet.  Exact fp32.  Purely additive to ABI 16.
 *
 *   sbc_link_code_create   base [rows][cols] circulant shifts (-1 = zero block), lifting size Z, interleaver P [N] (0-based:
 *                          bitsInt[i] = bitsEnc[P[i]]); N = cols Z, M = rows Z, K = N - M.  The handle owns the bit-packed generator
 *                          B^-1 A (H = [A | B]; the codeword is [payload; parity] with H c = 0), the edge tables and the workspace of
 *                          sbc_link_simulate, on the current device.  SBC_ERR_UNSUPPORTED: singular B, N > 8192, a check of degree
 *                          > 8 or < 2, more than 32768 edges.
 *   sbc_link_encode        payload [Npk][K] bytes 0 / 1 -> codeword [Npk][N] bytes (or NULL) and symbols [Npk][uses][S] complex64,
 *                          uses = floor(N / 2S): interleave, drop the N - 2 S uses tail bits, QPSK (first bit of a pair = MSB; integers
 *                          0, 1, 2, 3 -> (-1+j, -1-j, 1+j, 1-j) / sqrt 2); symbol k is stream k mod S of use k div S.
 *   sbc_link_llr           y = Hp_ideal[idx] x + sqrt(noise_power) w per channel use, then for Hp_ideal and Hp_est, every stream and
 *                          bit  log(sum_{s: bit = 0} exp(-|y - Hp s|^2 / noise_power) / sum_{s: bit = 1} ...)  over all 4^S candidates, each
 *                          class as a log-sum-exp around its smallest metric; flattened bit + 2 stream + 2S use, padded with zeros,
 *                          deinterleaved (out[P[j]] = flat[j]) and, unless SBC_LINK_NO_CLIP, clipped |l| >= 6 -> +-6.  Hp [pool][Nr][S]
 *                          complex64 (H Pt), chan_index [Npk][uses] int32 in [0, pool) (an index outside gives NaN soft bits, no read
 *                          out of bounds), w [Npk][uses][Nr] standard CN(0, 1).  S in {2, 4}, 1 <= Nr <= 64.
 *   sbc_link_decode        flooding sum-product on llr [Npk][N], check nodes in the exact pairwise form
 *                          a [+] b = sign a sign b min(|a|, |b|) + log1p(e^-|a+b|) - log1p(e^-|a-b|) as a forward / backward recursion;
 *                          at most max_iters iterations, with early_stop != 0 a codeword stops after the first iteration whose hard
 *                          decisions (total < 0 -> 1) satisfy every check.  soft [Npk][K]; totals [Npk][N] and iters [Npk] or NULL.
 *   sbc_link_errors        payload_hat = (sign(-soft) + 1) / 2 against payload: ber [Npk] (a soft output of 0 is an error), bler [Npk].
 *   sbc_link_simulate      encode -> llr -> decode x 2 -> errors for one chunk of packets at one SNR point, on the handle's workspace
 *                          (grown, with a device synchronisation, only when a larger chunk than ever before arrives).
 *
 * Randomness: caller buffers (payload, chan_index, noise are inputs), or with SBC_LINK_DEVICE_RANDOM the library's Philox4x32-10,
 * key = seed, counter (q, 4 snr_index + purpose, packet lo, packet hi) with packet = packet0 + position in the chunk -- a packet's draws
 * do not depend on chunking.  purpose 0: payload bit k = bit (k & 31) of word (k >> 5) & 3 of block q = k >> 7;  purpose 1: draw t = word
 * t & 3 of block t >> 2, index = (draw * pool) >> 32, without replacement when pool >= uses (a draw that repeats an earlier index of the
 * packet is skipped) and with replacement otherwise;  purpose 2: w of element e = use Nr + r as csrc/philox.h::complex_normal.  The
 * buffers are then outputs (noise may be NULL).  noise.py::link_streams replays them on the host.
 * Every launch is asynchronous on `stream`; every descriptor is checked before the first launch.  A packet's results are bit-identical
 * whatever the chunk and its position in it. */
#define SBC_LINK_DEVICE_RANDOM 1
#define SBC_LINK_NO_CLIP 2
typedef struct sbc_link_code sbc_link_code;
typedef struct sbc_link_code_desc {
    const int32_t* base;           /* [rows][cols]                                                              */
    const int32_t* interleaver;    /* [cols * Z]                                                                */
    int32_t rows, cols, Z;
} sbc_link_code_desc;
typedef struct sbc_link_random {
    uint64_t seed;
    int64_t packet0;               /* global index of the chunk's first packet                                  */
    int32_t snr_index;
    int32_t flags;                 /* SBC_LINK_DEVICE_RANDOM | SBC_LINK_NO_CLIP                                   */
} sbc_link_random;
typedef struct sbc_link_encode_desc {
    void* payload;                 /* [Npk][K] uint8: in, or out with SBC_LINK_DEVICE_RANDOM                    */
    void* codeword;                /* [Npk][N] uint8 out, or NULL                                               */
    void* symbols;                 /* [Npk][uses][S] complex64 out                                              */
    int32_t Npk, S;
    sbc_link_random rnd;
} sbc_link_encode_desc;
typedef struct sbc_link_llr_desc {
    const void* symbols;           /* [Npk][uses][S] complex64                                                  */
    const void* Hp_ideal;          /* [pool][Nr][S] complex64                                                   */
    const void* Hp_est;            /* [pool][Nr][S] complex64                                                   */
    void* chan_index;              /* [Npk][uses] int32: in, or out with SBC_LINK_DEVICE_RANDOM                 */
    void* noise;                   /* [Npk][uses][Nr] complex64: in, or out / NULL with SBC_LINK_DEVICE_RANDOM  */
    void* llr_ideal;               /* [Npk][N] float out                                                        */
    void* llr_est;                 /* [Npk][N] float out                                                        */
    float noise_power;
    int32_t Npk, pool, Nr, S;
    sbc_link_random rnd;
} sbc_link_llr_desc;
typedef struct sbc_link_sim_desc {
    const void* Hp_ideal;
    const void* Hp_est;
    void* payload;                 /* as sbc_link_encode_desc                                                   */
    void* chan_index;              /* as sbc_link_llr_desc                                                      */
    void* noise;
    void* ber_ideal;               /* [Npk] float out, each                                                     */
    void* bler_ideal;
    void* ber_est;
    void* bler_est;
    void* iters_ideal;             /* [Npk] int32 out or NULL, each                                             */
    void* iters_est;
    float noise_power;
    int32_t Npk, pool, Nr, S, max_iters;
    sbc_link_random rnd;
} sbc_link_sim_desc;
int sbc_link_code_create(const sbc_link_code_desc* desc, sbc_link_code** out);
void sbc_link_code_destroy(sbc_link_code* code);
int sbc_link_encode(sbc_link_code* code, const sbc_link_encode_desc* desc, void* stream);
int sbc_link_llr(sbc_link_code* code, const sbc_link_llr_desc* desc, void* stream);
int sbc_link_decode(sbc_link_code* code, const float* llr, int32_t Npk, int32_t max_iters, int32_t early_stop, float* soft, float* totals,
                    int32_t* iters, void* stream);
int sbc_link_errors(sbc_link_code* code, const float* soft, const void* payload, int32_t Npk, float* ber, float* bler, void* stream);
int sbc_link_simulate(sbc_link_code* code, const sbc_link_sim_desc* desc, void* stream);

/* ---- Environment variables -------------------------------------------------------------------------------------------------
 * Everything the library (csrc/) and the Python host (score_based_channels_amd/) read from the environment, in ONE place.  None of them
 * changes a result beyond the stated tolerance of the tests that set them; they configure the process or are needed by a test or by
 * bench.py.  Kernel selection and launch plans do not depend on the environment otherwise.  The torchrun variables RANK / WORLD_SIZE /
 * LOCAL_RANK are read by shard.py.  tests/test_host_logic.py::test_documented_environment_variables holds this list to the getenv /
 * os.environ sites of the tree.
 *
 *   process:    SBC_LIB_PATH (another build of this library), SBC_DIST_BACKEND (nccl | gloo; gloo lets several ranks share one GPU),
 *               SBC_DIST_TIMEOUT_S (bench.py: process-group timeout), SBC_CPU_BASELINE_WORKERS (bench.py: worker count of the cpu_baseline leg)
 *   tests:      SBC_STREAM_LAG_MIN_STEPS (driver.run_concurrently: fewest steps for which the second stream is lagged),
 *               SBC_NO_CALIB (scorenet.py: f16x2 activation scales stay 1)
 *   bench.py:   SBC_NO_CONV_DP_NORM (conv_dp.hip: the 64 -> 64 layers with a norm prologue / tile-moment output on the Winograd kernel;
 *               bench.py names the kernel of its roofline record by it)
 */

#ifdef __cplusplus
}
#endif
#endif /* SBC_HIP_H */
