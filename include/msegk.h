/*
 * msegk.h -- C ABI of libmsegk.so: the MI355X (gfx950) kernels behind the
 * medicalseg VNet hot path.
 *
 * The reference (PaddleCV-SIG/MedicalSeg) has no FFI of its own: its "operator
 * API" is the set of paddle.* calls made by medicalseg/models/vnet.py,
 * the medicalseg/models/losses modules, medicalseg/core/train.py and the
 * tools/preprocess_utils modules.  Each entry point below names the reference call
 * site(s) it replaces (file:line relative to the reference root).  The Python
 * package medicalseg_amd binds these with ctypes (medicalseg_amd/_lib.py); see
 * INTEGRATION.md for the stub a reference maintainer would add.
 *
 * Conventions
 *   - every function returns int: 0 = ok, <0 = error (msk_last_error() has text);
 *   - tensors are caller-owned DEVICE pointers described by msk_tensor:
 *     fp32, NDHWC, `ld` floats between consecutive voxels (ld >= c lets a tensor
 *     be a channel slice of a wider buffer -> zero-copy concat);
 *   - weights cross the boundary in the reference's layouts
 *     (Conv3D [Cout,Cin,kD,kH,kW]; Conv3DTranspose [Cin,Cout,kD,kH,kW]);
 *   - all launches are asynchronous on the context's stream; msk_sync blocks;
 *   - one context per device per process; a context is not thread-safe.
 */
#ifndef MSEGK_H
#define MSEGK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct msk_ctx msk_ctx;

typedef struct {
  void* p;                 /* device pointer to element (n=0,d=0,h=0,w=0,c=0) */
  int32_t n, d, h, w, c;   /* logical dims */
  int32_t ld;              /* floats per voxel in memory (>= c) */
} msk_tensor;

typedef struct {
  int32_t kd, kh, kw;      /* kernel */
  int32_t sd, sh, sw;      /* stride */
  int32_t pd, ph, pw;      /* zero padding (Conv3D only; 0 for Conv3DTranspose) */
} msk_conv_desc;

/* ---- context / memory ----------------------------------------------------- */
int msk_version(void);
int msk_device_count(int* count);
int msk_ctx_create(int device, msk_ctx** out);
int msk_ctx_destroy(msk_ctx* ctx);
const char* msk_last_error(msk_ctx* ctx);        /* ctx may be NULL (global error) */
int msk_sync(msk_ctx* ctx);
/* Weight-gradient kernels run on an internal side stream (option "wgrad_async"); msk_join_side makes
 * the main stream wait for them -- call it before consuming weight gradients (optimizer, all-reduce).
 * msk_sync and msk_d2h join implicitly. */
int msk_join_side(msk_ctx* ctx);
int msk_device_name(msk_ctx* ctx, char* buf, int buflen);
/* PCI bus id of the context's device ("0000:05:00.0"): the rank -> GPU binding a multi-rank job logs (parallel.py) */
int msk_device_pci_bus_id(msk_ctx* ctx, char* buf, int buflen);
int msk_malloc(msk_ctx* ctx, size_t bytes, void** out);
int msk_free(msk_ctx* ctx, void* p);
int msk_memset(msk_ctx* ctx, void* p, int value, size_t bytes);
/* Packed-weight cache contract.  The 5x5x5 / 3x3x3 convolution pipeline keeps a transformed, packed copy of every weight
 * tensor it has seen (keyed by its device address).  Every entry point of this library that WRITES caller memory
 * (msk_h2d*, msk_d2d, msk_memset, msk_sgd_momentum, msk_adam, msk_conv_fold_bn, msk_dp_allreduce_*, msk_dp_broadcast)
 * invalidates the copies of the bytes it writes, and msk_free drops those inside the freed allocation.  A caller that
 * changes weights ANY OTHER WAY (its own kernel or hipMemcpy on the buffer, or a library pass such as msk_copy_scale /
 * msk_interp_* / msk_ndhwc_to_ncdhw aimed at a weight tensor) must report the range here before the next convolution that
 * reads it; without the call that convolution would run with the stale packed weights (forward, data gradient and the
 * fused inference path -- the weight gradient never reads packed weights).  Cheap: a host-side table walk, no launch. */
int msk_weights_changed(msk_ctx* ctx, const void* p, size_t bytes);
/* host (pageable) -> device, ordered on the compute stream; src may be reused as soon as the call returns.
 * 64 KB .. 64 MB (the per-iteration batch upload of core/train.py:122-124) go through two internal pinned staging
 * buffers and do NOT synchronise the stream; other sizes copy and synchronise. */
int msk_h2d(msk_ctx* ctx, void* dst, const void* src, size_t bytes);
int msk_d2h(msk_ctx* ctx, void* dst, const void* src, size_t bytes);  /* synchronises the stream */
/* asynchronous host->device copy from PINNED memory (msk_pinned_alloc): returns immediately, the
 * source must stay untouched until the stream passes the copy (tools/prepare.py:200-259 loader path) */
int msk_h2d_async(msk_ctx* ctx, void* dst, const void* pinned_src, size_t bytes);
int msk_d2d(msk_ctx* ctx, void* dst, const void* src, size_t bytes);
int msk_pinned_alloc(msk_ctx* ctx, size_t bytes, void** out);
int msk_pinned_free(msk_ctx* ctx, void* p);
int msk_mem_info(msk_ctx* ctx, size_t* free_bytes, size_t* total_bytes);

/* ---- timing / profiling (HIP events on the context stream) ---------------- */
int msk_timer_start(msk_ctx* ctx);               /* records an event */
int msk_timer_stop(msk_ctx* ctx, float* ms);     /* records + synchronises; elapsed ms */
/* numbered marks on the compute stream: per-step times of a
 * run without a host synchronisation inside it (the reference's per-iteration batch_cost, core/train.py:172-173)        */
int msk_mark(msk_ctx* ctx, int idx /* 0..1023 */);
int msk_mark_elapsed(msk_ctx* ctx, int a, int b, float* ms);   /* waits for mark b */
/* ctx's compute stream waits (on the device, no host synchronisation) for everything enqueued so far on `other`'s compute
 * stream.  A second context = a second stream: the in-loop preprocessing of the NEXT sample (pinned H2D -> normalise ->
 * resample, tools/prepare_mri_spine_seg.py:71-80) runs there beside the training step and is handed over with two of these
 * (tools/bench_workloads.py --inloop-preprocess).  Both contexts must be on the same device. */
int msk_ctx_wait(msk_ctx* ctx, msk_ctx* other);
/* per-kernel profile: when enabled every launch is bracketed by events and its
 * duration accumulated under the kernel's tag.  The launches of the Winograd matrix stage (wbf_gemm_*) carry their events ON
 * the dispatch (hipExtLaunchKernelGGL start / stop events) instead of between two marker packets, which idle the queue for
 * ~6 us each; options: "prof_only_halo" 1 = only those launches (bench.py's roofline kernel), "prof_paused" 1 = take no events
 * until it is set back (no drain, no host synchronisation: sampling every Nth step), "prof_attach" 0 = marker brackets. */
int msk_prof_enable(msk_ctx* ctx, int on);
int msk_prof_reset(msk_ctx* ctx);
/* writes "tag\tcalls\ttotal_ms\n" lines into buf (NUL terminated); returns needed size via *len */
int msk_prof_report(msk_ctx* ctx, char* buf, int buflen, int* len);
/* knobs (debugging / A-B measurements; 0 = the product dispatch):
 *   "conv_impl": 1=VALU reference kernels everywhere, 3=reference wgrad only, 4=reference gather-conv only,
 *     5=no LDS wgrad, 6=no k==s scatter / forward-gather kernels, 7=scatter kernel at any size and the general gather
 *     kernel for the k==s forward convs, 8=no tight-K kernel,
 *     9=one-voxel VALU kernel for 32->ncls, 10=Winograd forward kernel even for tiny grids, 11=direct (non-Winograd)
 *     forward/data-gradient kernels, 12=fp32 Winograd weight gradient forced, 13=direct weight-gradient kernels,
 *     14=fp32 Winograd F(2,5) instead of F(4,5), 16=tap-row weight-gradient kernel for the kernel == stride convolutions,
 *     20=fp32-MFMA Winograd kernels instead of the bf16x3 pipeline, 21=the same for the weight gradient only,
 *     22=VALU kernel instead of the folded-column MFMA kernel for 32->ncls (conv_foldn_k), 23=VALU kernel instead of
 *     conv_c1_mfma_k for 1->16, 24=fp32-MFMA form of conv_foldn_k instead of the fp16 two-piece form,
 *     25=fp32-MFMA tight-K kernel instead of conv_tk_h2_k for ncls->32,
 *     26=fp32-MFMA (tap, class)-row weight gradient instead of wgrad_cbs_h2_k for 32->ncls;
 *   "wino_bf3" 0|1 (0 = fp32-MFMA Winograd kernels everywhere; also env MSEGK_WBF=0), "wbf_variant" (-1 auto | tile variant
 *     of wbf_gemm_k), "wbf_tin_map" 0|1 (lane mapping of the transform kernel);
 *   "wgrad_async" 0|1 (weight gradients on the side stream), "wgrad_async_max_m" (voxel limit for it, 0 = all);
 *   "prof_shapes" 0|1, "prof_only_halo" 0|1 (profile only the 5^3 halo-conv kernels), "poison_scratch" byte|-1;
 *   "direct_conv" 0|1 (1 = no Winograd kernels; also env MSEGK_DIRECT_CONV=1);
 *   "conv_split" 3|2: operand split of the Winograd pipelines: 3 = three bf16 pieces (exact fp32 operands, six MFMAs per
 *     product), 2 = two fp16 pieces with a scaled residual (22 significand bits, three MFMAs per product; gradients are
 *     scaled by a power of two derived on the device, forward activations must stay below 3000 in magnitude);
 *   "bwd_fuse" -1|0|1|2 (msk_conv3d_bwd_bnact: auto | three calls | one dual transform | one transform per stream),
 *     "foldn_wgs" (workgroups per CU targeted by the D segmentation of conv_foldn_k, 0 = 2);
 *     "tk_join" 1|0 (msk_conv3d_bwd_bnact_join: 1 = the join backward runs in the data-gradient kernel's epilogue, 0 = it declines);
 *     "affine_map" 1|0 (msk_affine_patch: 1 = a wavefront covers a 2 x 2 x 16 box of the patch, 0 = row-linear; same results);
 *     "topk_agg_hist" 0|1 (msk_topk_*: 1 = the first histogram pass adds a wavefront's lanes of one bin with one LDS atomic instead of one per lane; same results);
 *     "wbf_pad_min_voxels" (smallest 5^3 problem whose channel counts are not multiples of 32 that is run through the
 *         16-bit pipeline on a zero-padded copy, default 2^18);
 *     "wbf_tin_groups" (workgroups below which the pipeline's transform kernels cut their W tiles into chunks, -1 = 8 per CU, 0 = never);
 *     "tile_staging" 0|1 (dense 5..32-channel voxel records -- the 20-class 1x1x1 head and its loss kernels -- through an LDS tile with
 *         whole-line accesses; 0 = one thread per voxel straight from HBM, bitwise the same results), "kst_pair" 0|1 (gconv_kst_k:
 *         both h-parity classes of <= 16 output channels in one matrix instruction);
 *     "reduce_vpl" (voxels per lane the per-channel reduction kernels aim for before they add workgroups, default 8),
 *         "reduce_vpl_site" (site * 1000 + voxels per lane for ONE family of reductions -- 0 forward statistics, 1 BatchNorm backward
 *         sums, 2 joins, 3 channel sums; 0 = follow "reduce_vpl" -- another summation order of the same sums: the full-size parity
 *         test measures the distance between two fp32 evaluations of a step with it);
 *   tuning: "halo_tile" / "wgrad_chunk" (-1 auto or table index), "wgrad_rounds" / "wgrad_wino_rounds" (workgroups
 *   per CU targeted by the split-K of the direct / Winograd weight-gradient kernels; "wgrad_wino_rounds" 0 = pick the
 *   split count that fills whole waves of resident workgroups, the default) */
int msk_set_option(msk_ctx* ctx, const char* key, int value);
/* effective value of "dp_mode" (after MSEGK_DP_MODE and msk_dp_init's fall-backs), "conv_split", "wgrad_async", "world", "rank",
 * "num_cu", "scalar_ring_served"; and the launch geometry of the elementwise kernels as it stands: "ew_cap", "reduce_cap",
 * "reduce_vpl", "dense12" (what a caller that changes them puts back) */
int msk_get_option(msk_ctx* ctx, const char* key, int* value);

/* ---- layout at the boundary ------------------------------------------------ */
/* NCDHW (reference layout, core/train.py:123) <-> NDHWC (device layout) */
int msk_ncdhw_to_ndhwc(msk_ctx* ctx, const float* src, msk_tensor dst);
int msk_ndhwc_to_ncdhw(msk_ctx* ctx, msk_tensor src, float* dst);

/* ---- convolutions ---------------------------------------------------------- */
/* paddle.nn.Conv3D forward   (models/vnet.py:36,67-68,98-99,165-166,169)
 *   y[N,OD,OH,OW,Cout] = conv(x[N,ID,IH,IW,Cin], w[Cout,Cin,k]) + bias        */
int msk_conv3d_fwd(msk_ctx* ctx, msk_conv_desc cd, msk_tensor x, const float* w,
                   const float* bias /*nullable*/, msk_tensor y);
/* Inference path (core/infer.py:62-94, core/val.py:89-110 run the net in eval mode): the chain
 * Conv3D -> BatchNorm3D(running statistics) -> PReLU of vnet.py:36-41 as ONE convolution.
 *   msk_conv_fold_bn:    w'[co][...] = w[co][...] * scale[co];  b'[co] = b[co] * scale[co] + shift[co]
 *                        (scale/shift from msk_bn_eval_coeffs; w canonical [Cout][inner = Cin * taps]; bias nullable)
 *   msk_conv3d_fwd_act:  y = PReLU_slope(conv(x, w) + bias); the Winograd kernels apply the slope in their epilogue,
 *                        every other kernel is followed by one in-place pass (same result).  slope nullable.        */
int msk_conv_fold_bn(msk_ctx* ctx, const float* w, const float* bias, const float* scale, const float* shift,
                     int cout, long inner, float* w_folded, float* b_folded);
int msk_conv3d_fwd_act(msk_ctx* ctx, msk_conv_desc cd, msk_tensor x, const float* w, const float* bias,
                       const float* prelu_slope, msk_tensor y);
/* Training-path forms of Conv3D forward / weight gradient for the conv -> BatchNorm units of vnet.py:36-41:
 *   msk_conv3d_fwd_ex:   as msk_conv3d_fwd; additionally
 *       stats_local (nullable): BatchNorm statistics of y (the msk_bn_stats record, mean[Cout] then M2[Cout]) -- taken in
 *                    the convolution's output stage when the kernel supports it (no second read of y), else by msk_bn_stats;
 *       xform (nullable): caller-owned device buffer of msk_conv3d_xform_bytes() bytes that receives the transformed input
 *                    (Winograd B^T x, split into bf16 pieces) the convolution computes anyway; it stays valid while x is
 *                    unchanged.  Pass it only when msk_conv3d_xform_bytes() > 0.  For the 32 -> ncls <= 3 class
 *                    (out_tr.conv1, vnet.py:165) the buffer is 512 bytes: only max |x|, which the fp16 two-piece forward
 *                    kernel measures anyway, travels to the weight gradient.
 *   msk_conv3d_wgrad_ex: as msk_conv3d_wgrad; xform (nullable) = the buffer msk_conv3d_fwd_ex filled for the SAME x,
 *                    which saves recomputing the transform of x (the layer input kept for backward, vnet.py:41).
 *   msk_conv3d_xform_bytes: size of that buffer for input x and cout output channels; 0 = the convolution does not
 *                    produce one (pass NULL).                                                              */
size_t msk_conv3d_xform_bytes(msk_ctx* ctx, msk_conv_desc cd, msk_tensor x, int cout);
int msk_conv3d_fwd_ex(msk_ctx* ctx, msk_conv_desc cd, msk_tensor x, const float* w, const float* bias /*nullable*/,
                      msk_tensor y, float* stats_local /*nullable*/, void* xform /*nullable*/);
int msk_conv3d_wgrad_ex(msk_ctx* ctx, msk_conv_desc cd, msk_tensor x, msk_tensor dy, float* dw, float* db /*nullable*/,
                        int accumulate, const void* xform /*nullable*/);
/* "amax arrays" (round 3): the fp16 two-piece convolution pipeline scales every operand tensor by a power of two taken from
 * its max |value|.  For a layer input that maximum can ride along in the pass that PRODUCES the tensor (bn1/relu1 of the
 * previous LUConv, vnet.py:41; the residual joins :110-111,154; the Dropout3D copies :102,147-148) instead of costing a
 * read of its own:
 *   msk_amax_new            n consecutive zeroed device arrays of 64 floats whose maximum counts (from a ring: valid for
 *                           the next ~500 requests, i.e. well beyond the training step that uses them);
 *   msk_*_amax              as the entry point without the suffix, and max |written values| is folded into out_amax
 *                           (nullable; several calls may fold into the same array: the two halves of a concat buffer);
 *   msk_conv3d_fwd_ex2      as msk_conv3d_fwd_ex with x_amax (nullable) = such an array covering all of x.        */
float* msk_amax_new(msk_ctx* ctx, int n /* consecutive arrays */);
int msk_conv3d_fwd_ex2(msk_ctx* ctx, msk_conv_desc cd, msk_tensor x, const float* w, const float* bias /*nullable*/,
                       msk_tensor y, float* stats_local /*nullable*/, void* xform /*nullable*/, const float* x_amax /*nullable*/);
int msk_affine_act_fwd_amax(msk_ctx* ctx, msk_tensor x, const float* scale, const float* shift, msk_tensor res,
                            const float* alpha, msk_tensor out, float* out_amax);
int msk_affine_act_join_fwd_amax(msk_ctx* ctx, msk_tensor y, const float* scale, const float* shift, const float* alpha_inner,
                                 msk_tensor res, const float* alpha_outer, msk_tensor out, float* out_amax);
int msk_copy_scale_amax(msk_ctx* ctx, msk_tensor src, const float* mask, msk_tensor dst, int accumulate, float* dst_amax);
/* the gradient side of the same idea: dy_amax (nullable) = the amax array the pass that wrote dy folded max |dy| into
 * (msk_affine_act_bwd_apply_amax); msk_conv3d_wgrad_ex2 otherwise as msk_conv3d_wgrad_ex.                        */
int msk_conv3d_dgrad_ex(msk_ctx* ctx, msk_conv_desc cd, msk_tensor dy, const float* w, msk_tensor dx, int accumulate,
                        const float* dy_amax /*nullable*/);
int msk_conv3d_wgrad_ex2(msk_ctx* ctx, msk_conv_desc cd, msk_tensor x, msk_tensor dy, float* dw, float* db /*nullable*/,
                         int accumulate, const void* xform /*nullable*/, const float* dy_amax /*nullable*/);
/* ... and x_amax (nullable): the amax array of x from the pass that produced it, used when no kept transform brings the scale */
int msk_conv3d_wgrad_ex3(msk_ctx* ctx, msk_conv_desc cd, msk_tensor x, msk_tensor dy, float* dw, float* db /*nullable*/,
                         int accumulate, const void* xform /*nullable*/, const float* dy_amax /*nullable*/, const float* x_amax /*nullable*/);
/* Launch diet (round 3): the per-channel epilogues of a BatchNorm layer ride in the merge kernels that precede them.
 *   msk_bn_fin              the arguments of msk_bn_finalize(world = 1, count) as a struct;
 *   msk_conv3d_fwd_ex3      msk_conv3d_fwd_ex2, and with fin != NULL (stats_local required) the finalisation runs in the
 *                           launch that merges the statistics: bitwise the results of msk_conv3d_fwd_ex2 + msk_bn_finalize.
 *                           (SyncBatchNorm over several ranks keeps the separate calls: an all-gather sits between them.)
 *   msk_bn_stats_fin        msk_bn_stats + msk_bn_finalize(world = 1) the same way (the up-convolutions, vnet.py:150);
 *   msk_affine_act_bwd_reduce_pg / msk_add_act_join_bwd_pg
 *                           as the _ex forms, and the parameter gradients msk_affine_act_param_grads would take from the
 *                           sums are ADDED to dgamma / dbeta / dalpha (nullable) in the launch that merges the sums;
 *                           clear_maxes = 0: `maxes` arrives zeroed (msk_amax_new(ctx, 2)), no memset is enqueued.        */
typedef struct msk_bn_fin {
  const float* gamma; /* nullable */
  const float* beta;  /* nullable */
  float eps, momentum;
  double count;       /* values per channel (N*D*H*W) */
  float* running_mean; /* nullable */
  float* running_var;  /* nullable */
  float* save_mean;
  float* save_invstd;
  float* scale;        /* NULL = no finalisation */
  float* shift;
} msk_bn_fin;
int msk_conv3d_fwd_ex3(msk_ctx* ctx, msk_conv_desc cd, msk_tensor x, const float* w, const float* bias /*nullable*/,
                       msk_tensor y, float* stats_local /*nullable*/, void* xform /*nullable*/, const float* x_amax /*nullable*/,
                       const msk_bn_fin* fin /*nullable*/);
int msk_bn_stats_fin(msk_ctx* ctx, msk_tensor x, float* stats_local, const msk_bn_fin* fin /*nullable*/);
/* Convolution followed by INSTANCE statistics (paddle.nn.InstanceNorm3D: per (sample, channel) over D*H*W; the builder-defined
 * UNet3D of BASELINE configs[3]): stats is [N][2 Cout]; fin describes sample 0 (count = D*H*W, running_* ignored when NULL) and
 * sample n's save_mean / save_invstd / scale / shift lie fin_stride floats further per sample.  When the convolution kernel
 * keeps per-tile records (the one-kernel matrix stage, <= 64 channels) the N merges read those; otherwise one statistics pass
 * per sample runs on y -- the results are the same to fp32 rounding either way.                                              */
int msk_conv3d_fwd_in(msk_ctx* ctx, msk_conv_desc cd, msk_tensor x, const float* w, const float* bias /*nullable*/, msk_tensor y,
                      float* stats, void* xform /*nullable*/, const float* x_amax /*nullable*/, const msk_bn_fin* fin,
                      int fin_stride);
int msk_affine_act_bwd_reduce_pg(msk_ctx* ctx, msk_tensor x, const float* scale, const float* shift, msk_tensor res,
                                 const float* alpha, const float* mean, const float* invstd, msk_tensor dout, float* sums,
                                 float* maxes /*nullable*/, int clear_maxes, float* dgamma, float* dbeta, float* dalpha);
int msk_add_act_join_bwd_pg(msk_ctx* ctx, msk_tensor y, const float* scale, const float* shift, const float* alpha_inner,
                            msk_tensor res, const float* alpha_outer, const float* mean, const float* invstd, msk_tensor dout,
                            msk_tensor da, msk_tensor dres, int dres_accumulate, float* dalpha_outer, float* unit_sums,
                            float* maxes /*nullable*/, int clear_maxes, float* unit_dgamma, float* unit_dbeta, float* unit_dalpha);
/* Backward of one conv -> BatchNorm(batch statistics) -> PReLU unit (LUConv, vnet.py:36-41; autograd of core/train.py:139)
 * in one call:   dy = msk_affine_act_bwd_apply(y, ..., dout, sums_total, M_total, bn_mode 1, no residual),
 *                dx (+)= conv^T(dy, w)   (dx.p NULL -> skipped),   dw (+)= sum dy * x.
 * When both gradients run on the transform pipeline (square 5^3 / 3^3 'same' layers; msk_conv3d_bwd_bnact_bytes() > 0) dy is
 * evaluated inside the kernel that writes its two transforms and never reaches HBM: then `ybuf` (caller-owned,
 * msk_conv3d_bwd_bnact_bytes() bytes, must stay untouched until the weight gradient -- possibly on the side stream -- has
 * run, i.e. until the next msk_sync / optimizer step) receives the second transform and `dy_scratch` is not written.
 * Otherwise (ybuf NULL, or the shape is not eligible) the three operations run one after the other with dy in `dy_scratch`
 * (a tensor of y's shape, required either way).  xform as in msk_conv3d_wgrad_ex.  Results agree with the separate calls
 * to fp32 rounding.  A convolution with ONE input channel and dx.p NULL (in_tr.conv1, vnet.py:67) evaluates dy inside its
 * weight-gradient kernel as well (no ybuf / xform / maxes needed; dy_scratch is not written), on the calling stream.  */
size_t msk_conv3d_bwd_bnact_bytes(msk_ctx* ctx, msk_conv_desc cd, msk_tensor x, msk_tensor y);
int msk_conv3d_bwd_bnact(msk_ctx* ctx, msk_conv_desc cd, msk_tensor x, const float* w, msk_tensor y, const float* scale,
                         const float* shift, const float* alpha /*nullable*/, const float* mean, const float* invstd,
                         const float* gamma, msk_tensor dout, const float* sums_total, double M_total,
                         msk_tensor dy_scratch, msk_tensor dx, int dx_accumulate, float* dw, int dw_accumulate,
                         const void* xform /*nullable*/, void* ybuf /*nullable*/,
                         const float* maxes /*nullable: msk_affine_act_bwd_reduce_ex's, needed by the fused forms under "conv_split" 2*/);
/* msk_conv3d_bwd_bnact for the layer behind a zero-copy concat (UpTransition.ops[0]: x = the concat buffer, vnet.py:152-154).
 * dx accumulates into the interleaved gradient buffer as usual UNLESS the one-kernel matrix stage runs the data gradient: then
 * the sums (old dx + new) are STORED to the two dense half tensors dx_lo / dx_hi (channels [0, c/2) / [c/2, c), voxel stride
 * c/2) and *split_done = 1 -- the consumers of the halves (the up-convolution's and the skip's backward) read dense voxels
 * instead of one half of every 128-byte line.  *split_done = 0: dx holds the result, dx_lo / dx_hi are untouched. */
int msk_conv3d_bwd_bnact_split(msk_ctx* ctx, msk_conv_desc cd, msk_tensor x, const float* w, msk_tensor y, const float* scale,
                               const float* shift, const float* alpha /*nullable*/, const float* mean, const float* invstd,
                               const float* gamma, msk_tensor dout, const float* sums_total, double M_total,
                               msk_tensor dy_scratch, msk_tensor dx, int dx_accumulate, float* dw, int dw_accumulate,
                               const void* xform /*nullable*/, void* ybuf /*nullable*/, const float* maxes /*nullable*/,
                               msk_tensor dx_lo, msk_tensor dx_hi, int* split_done);
/* msk_conv3d_bwd_bnact(_split) whose accumulating data gradient takes its OLD values from another tensor, dx_old (geometry and voxel
 * stride of dx), and writes the sums to dx (or to the dense halves dx_lo / dx_hi when the one-kernel matrix stage runs it:
 * *split_done = 1).  The residual joins of vnet.py:110-111,154 hand one gradient to both operands: msk_add_act_bwd /
 * msk_add_act_join_bwd_* accept a null second destination, and the layer behind the join reads the first one here -- one full
 * write of the tensor less per join.  dx_old.p == NULL: msk_conv3d_bwd_bnact(_split).  dx_lo / dx_hi / split_done may be null. */
int msk_conv3d_bwd_bnact_acc(msk_ctx* ctx, msk_conv_desc cd, msk_tensor x, const float* w, msk_tensor y, const float* scale,
                             const float* shift, const float* alpha, const float* mean, const float* invstd, const float* gamma,
                             msk_tensor dout, const float* sums_total, double M_total, msk_tensor dy_scratch, msk_tensor dx,
                             int dx_accumulate, float* dw, int dw_accumulate, const void* xform, void* ybuf, const float* maxes,
                             msk_tensor dx_old, msk_tensor dx_lo, msk_tensor dx_hi, int* split_done);
/* Backward of a unit conv5^3 -> BatchNorm(batch statistics) -> PReLU with <= 4 output channels whose 32-channel input x is the
 * output of a residual join fused with ITS unit, out = prelu(prelu(jscale * jy + jshift, jalpha_inner) + jres, jalpha_outer)
 * (out_tr.conv1 behind up_tr32's join, vnet.py:154,173), together with that join's backward, in one call:
 *     dy = msk_affine_act_bwd_apply_amax(y, ..., dout, sums_total, M_total, bn_mode 1) (dy_amax nullable),
 *     dw (+)= sum dy * x   (msk_conv3d_wgrad_ex3: xform / x_amax nullable),
 *     msk_add_act_join_bwd_pg(jy, ..., dout = conv^T(dy, w), da, dres, ...) with the same trailing arguments --
 * evaluated in the epilogue of the data-gradient kernel, so the join's output gradient is never stored.  da is bitwise what the
 * separate calls give; unit_sums and the parameter gradients differ by their summation order.  unit_sums needs 4*C floats
 * (C = x.c): [0..3C) = sum du, sum du*xhat, d alpha_inner, and the merge also stores the join's slope sum in [3C..4C).
 * dres.p NULL: the second operand's gradient is not written (it equals da: msk_conv3d_bwd_bnact_acc's dx_old).
 * Returns 0 = done, 1 = not eligible (NOTHING was launched: use the separate calls) -- an accumulate flag set, option "tk_join" 0, "conv_split" != 2,
 * a forced "conv_impl", x.c != 32, tensors that are not float4-aligned, volumes below 4 x 8 x 12.                          */
int msk_conv3d_bwd_bnact_join(msk_ctx* ctx, msk_conv_desc cd, msk_tensor x, const float* w, msk_tensor y, const float* scale,
                              const float* shift, const float* alpha /*nullable*/, const float* mean, const float* invstd,
                              const float* gamma, msk_tensor dout, const float* sums_total, double M_total, msk_tensor dy,
                              float* dy_amax /*nullable*/, float* dw, int dw_accumulate, const void* xform /*nullable*/,
                              const float* x_amax /*nullable*/, msk_tensor jy, const float* jscale, const float* jshift,
                              const float* jalpha_inner, msk_tensor jres, const float* jalpha_outer, const float* jmean,
                              const float* jinvstd, msk_tensor da, int da_accumulate, msk_tensor dres /*p nullable*/,
                              int dres_accumulate, float* dalpha_outer, float* unit_sums, float* maxes, int clear_maxes,
                              float* unit_dgamma /*nullable*/, float* unit_dbeta /*nullable*/, float* unit_dalpha /*nullable*/);
/* Backward of an up-convolution unit  convT -> BatchNorm(batch statistics) -> PReLU  (UpTransition.up_conv / bn1 / relu1,
 * vnet.py:133-150; autograd of core/train.py:139) behind its reduce pass, in one call:
 *     dx (+)= convT^T(dy, w),  dw (+)= sum x * dy,   dy = msk_affine_act_bwd_apply(y, ..., dout, sums_total, M_total, bn_mode 1)
 * where the data gradient evaluates dy from (y, dout) in its own loads (<= 16 output channels of the convT, kernel == stride)
 * and the pass that writes dy_scratch runs on the weight-gradient stream in front of the weight gradient, its only reader.
 * Returns 0 = done, 1 = not eligible (NOTHING was launched: use msk_affine_act_bwd_apply + msk_convT3d_wgrad / _dgrad). */
int msk_convT3d_bwd_bnact(msk_ctx* ctx, msk_conv_desc cd, msk_tensor x, const float* w, msk_tensor y, const float* scale,
                          const float* shift, const float* alpha /*nullable*/, const float* mean, const float* invstd,
                          msk_tensor dout, const float* sums_total, double M_total, msk_tensor dy_scratch, msk_tensor dx,
                          int dx_accumulate, float* dw, int dw_accumulate);
/* The in_tr.conv1 unit (vnet.py:57-79: out = PReLU(BN(conv5^3(x: ONE channel)) + tile(x)), no data gradient): weight gradient
 * with dy evaluated inside the kernel from (y, dout); `res` is either a null tensor or x itself (the tiled residual, read from the
 * kernel's own halo of x).  Returns 0 = done, 1 = not this class / declined (nothing was launched: use msk_affine_act_bwd_apply +
 * msk_conv3d_wgrad), < 0 = error.  Runs on the calling stream.                                                     */
/* The same unit with INSTANCE statistics (conv -> InstanceNorm -> PReLU; builder-defined UNet3D): sample n's scale / shift / mean /
 * invstd lie n * coef_stride floats after the given pointers, its sums (msk_affine_act_bwd_reduce* of that sample) n * sums_stride
 * floats, M_sample = D*H*W.  Only the fused form exists: returns 1 with NOTHING launched when it is not eligible (the caller then
 * runs msk_affine_act_bwd_apply per sample and the separate gradient calls), 0 when done.  maxes: the two amax arrays the
 * reduce passes of ALL samples folded into (required for the fp16 operand formats).                                         */
int msk_conv3d_bwd_inact(msk_ctx* ctx, msk_conv_desc cd, msk_tensor x, const float* w, msk_tensor y, const float* scale,
                         const float* shift, const float* alpha /*nullable*/, const float* mean, const float* invstd, int coef_stride,
                         msk_tensor dout, const float* sums, int sums_stride, double M_sample, msk_tensor dx, int dx_accumulate,
                         float* dw, int dw_accumulate, const void* xform, void* ybuf, const float* maxes /*nullable*/);
int msk_conv3d_bwd_bnact_c1(msk_ctx* ctx, msk_conv_desc cd, msk_tensor x, msk_tensor y, const float* scale, const float* shift,
                            const float* alpha /*nullable*/, const float* mean, const float* invstd, msk_tensor res,
                            msk_tensor dout, const float* sums_total, double M_total, float* dw, int dw_accumulate);
/* autograd of the above (core/train.py:139 loss.backward()):
 *   dx (+)= conv^T(dy, w);  accumulate != 0 adds into dx                       */
int msk_conv3d_dgrad(msk_ctx* ctx, msk_conv_desc cd, msk_tensor dy, const float* w,
                     msk_tensor dx, int accumulate);
/*   dw[Cout,Cin,k] (+)= sum_voxels dy * x ;  db[Cout] (+)= sum dy  (db nullable) */
int msk_conv3d_wgrad(msk_ctx* ctx, msk_conv_desc cd, msk_tensor x, msk_tensor dy,
                     float* dw, float* db /*nullable*/, int accumulate);
/* paddle.nn.Conv3DTranspose forward (models/vnet.py:133-137), w[Cin,Cout,k],
 * out = (in-1)*s + k                                                           */
int msk_convT3d_fwd(msk_ctx* ctx, msk_conv_desc cd, msk_tensor x, const float* w,
                    const float* bias /*nullable*/, msk_tensor y);
/* the same + the BatchNorm statistics of y for the unit UpTransition.up_conv -> bn1 (vnet.py:133-150): stats_local [2 C] = (mean, M2)
 * of this rank's values, fin (nullable) = msk_bn_finalize(world 1) in the merge launch -- taken in the convolution's store pass where
 * the kernel can (no separate read of y), by msk_bn_stats_fin otherwise.  Same results to fp32 rounding. */
int msk_convT3d_fwd_ex(msk_ctx* ctx, msk_conv_desc cd, msk_tensor x, const float* w, const float* bias, msk_tensor y,
                       float* stats_local, const msk_bn_fin* fin /*nullable*/);
int msk_convT3d_dgrad(msk_ctx* ctx, msk_conv_desc cd, msk_tensor dy, const float* w,
                      msk_tensor dx, int accumulate);
int msk_convT3d_wgrad(msk_ctx* ctx, msk_conv_desc cd, msk_tensor x, msk_tensor dy,
                      float* dw, float* db /*nullable*/, int accumulate);

/* ---- BatchNorm3D / SyncBatchNorm + PReLU + residual ------------------------- */
/* paddle.nn.BatchNorm3D -> SyncBatchNorm statistics (models/vnet.py:38,70,100,139,167;
 * cvlibs/config.py:322).  Welford/Chan merge, biased variance over N*D*H*W.
 * stats_local[2*C] = {mean[C], M2[C]} of THIS rank's x.                        */
int msk_bn_stats(msk_ctx* ctx, msk_tensor x, float* stats_local);
/* Merge `world` rank-local stats (gathered[world][2*C], equal counts `count_per_rank`)
 * into mean/var, write scale = gamma*invstd, shift = beta - mean*scale, save
 * mean[C], invstd[C]; running <- momentum*running + (1-momentum)*batch when
 * running_mean/var are non-NULL.                                               */
int msk_bn_finalize(msk_ctx* ctx, const float* gathered, int world, double count_per_rank,
                    int C, const float* gamma, const float* beta, float eps, float momentum,
                    float* running_mean, float* running_var, float* save_mean,
                    float* save_invstd, float* scale, float* shift);
/* eval mode: scale/shift from running statistics (model.eval(), core/val.py:57) */
int msk_bn_eval_coeffs(msk_ctx* ctx, int C, const float* gamma, const float* beta,
                       const float* running_mean, const float* running_var, float eps,
                       float* save_mean, float* save_invstd, float* scale, float* shift);
/* out = prelu(scale[c]*x + shift[c] + res, alpha[c])
 *   scale/shift NULL -> identity affine;  res.p NULL -> no residual;
 *   res.c < out.c -> residual channel = c % res.c (x.tile, vnet.py:78);
 *   alpha NULL -> no activation.  Replaces bn1/relu1/relu2/paddle.add chains
 *   (vnet.py:41,77-79,107-111,150-154,173).                                    */
int msk_affine_act_fwd(msk_ctx* ctx, msk_tensor x, const float* scale, const float* shift,
                       msk_tensor res, const float* alpha, msk_tensor out);
/* the same with the maximum of |out| folded into an amax array (msk_affine_act_fwd_amax) AND a second copy of the result in out2
 * (nullable; its own voxel stride): InputTransition writes its output into the skip half of the up-transition's concat buffer
 * (vnet.py:152) and, for the readers of that half alone, as a dense tensor -- a 16-channel half of a 32-channel voxel is 64 of
 * every 128-byte line.  Channel-stationary float4 kernel only (C / 4 a power of two). */
int msk_affine_act_fwd_amax2(msk_ctx* ctx, msk_tensor x, const float* scale, const float* shift, msk_tensor res,
                             const float* alpha, msk_tensor out, float* out_amax /*nullable*/, msk_tensor out2);
/* backward pass 1: per-channel sums over this rank:
 *   sums[0..C)   = sum du            (du = dout * (u>0 ? 1 : alpha))
 *   sums[C..2C)  = sum du * xhat     (xhat = (x-mean)*invstd; 0 if no BN)
 *   sums[2C..3C) = sum dout * u * [u<=0]   (d alpha)                           */
int msk_affine_act_bwd_reduce(msk_ctx* ctx, msk_tensor x, const float* scale, const float* shift,
                              msk_tensor res, const float* alpha, const float* mean,
                              const float* invstd, msk_tensor dout, float* sums);
/* the same; maxes (nullable, device float[2][64]: two "amax arrays" -- the maximum of each row counts, the kernel spreads
 * its atomics over the entries) additionally receives max |du| and max |xhat| over the tensor -- the bound
 * msk_conv3d_bwd_bnact needs to scale dy into fp16 range when option "conv_split" is 2.  Requires C % 4 == 0, voxel
 * strides % 4 == 0 and 16-byte aligned tensors.                                                              */
int msk_affine_act_bwd_reduce_ex(msk_ctx* ctx, msk_tensor x, const float* scale, const float* shift,
                                 msk_tensor res, const float* alpha, const float* mean,
                                 const float* invstd, msk_tensor dout, float* sums, float* maxes /*nullable*/);
/* backward pass 2: dx = BN-backward(du) and dres (+)= du.
 *   bn_mode 0: no BN (dx = du); 1: training BN (uses sums, total count M over all
 *   ranks); 2: eval BN (dx = scale*du).  dres.p NULL -> skipped; dres_acc adds.   */
int msk_affine_act_bwd_apply(msk_ctx* ctx, msk_tensor x, const float* scale, const float* shift,
                             msk_tensor res, const float* alpha, const float* mean,
                             const float* invstd, const float* gamma, msk_tensor dout,
                             const float* sums_total, double M_total, int bn_mode,
                             msk_tensor dx, msk_tensor dres, int dres_acc);
/* the same; dx_amax (nullable, an amax array of msk_amax_new) additionally receives max |dx| -- the gradient kernels of the
 * convolution in front (msk_conv3d_dgrad_ex / msk_conv3d_wgrad_ex2) then skip their own pass over dx.  One array may collect
 * several calls (per-sample InstanceNorm units): the maximum is associative.                                    */
int msk_affine_act_bwd_apply_amax(msk_ctx* ctx, msk_tensor x, const float* scale, const float* shift,
                                  msk_tensor res, const float* alpha, const float* mean,
                                  const float* invstd, const float* gamma, msk_tensor dout,
                                  const float* sums_total, double M_total, int bn_mode,
                                  msk_tensor dx, msk_tensor dres, int dres_acc, float* dx_amax /*nullable*/);
/* parameter gradients of the above from the (all-reduced) sums:
 *   dgamma (+)= sums[C..2C), dbeta (+)= sums[0..C), dalpha (+)= sums[2C..3C)     */
int msk_affine_act_param_grads(msk_ctx* ctx, int C, const float* sums, float* dgamma,
                               float* dbeta, float* dalpha, int accumulate);

/* ---- concat / dropout / small elementwise ---------------------------------- */
/* dst = src * mask[n*C+c] (mask NULL -> 1): paddle.concat slices (vnet.py:152) and
 * nn.Dropout3D with a given mask (vnet.py:103,144-145);  accumulate adds.       */
int msk_copy_scale(msk_ctx* ctx, msk_tensor src, const float* mask, msk_tensor dst, int accumulate);
/* counter-based Dropout3D mask: mask[n*C+c] = keep ? 1/(1-p) : 0, keyed by
 * (seed, step, site).                                                          */
int msk_dropout_mask(msk_ctx* ctx, uint64_t seed, uint64_t step, uint32_t site, int count,
                     float p, float* mask);
/* out[c] (+)= sum over voxels of x[..,c]  (bias gradients)                      */
int msk_channel_sum(msk_ctx* ctx, msk_tensor x, float* out, int accumulate);
/* paddle.argmax(logit, axis=1) (core/infer.py:92) */
int msk_argmax_c(msk_ctx* ctx, msk_tensor x, int32_t* out);
/* out[v][c] = softmax over c of x[v][:]  -- F.softmax(logits, axis=1) of the AUC path of evaluate (core/val.py:121-123)  */
int msk_softmax_c(msk_ctx* ctx, msk_tensor x, msk_tensor out);

/* ---- test-time augmentation (core/infer.py aug_inference) ------------------- */
/* dst = src mirrored along the axes of mask (bit 0 = D, bit 1 = H, bit 2 = W; per batch item, any c, any ld >= c), out of
 * place, in one pass: np.flip bit for bit.  mask 0 copies.                                                           */
int msk_flip_axes(msk_ctx* ctx, msk_tensor src, msk_tensor dst, int mask);
/* acc[v][c] = first ? p : acc[v][c] + p, p = msk_softmax_c's value (the same operations in the same order) of the logits
 * at the voxel v is mirrored to by mask: one pass of a flip-averaged prediction without the mirrored copy and the
 * probabilities in between.  The addition is an fp32 addition of its own, never fused with the softmax's multiply.    */
int msk_tta_accumulate(msk_ctx* ctx, msk_tensor logits, int mask, msk_tensor acc, int first);
/* probs[v][c] = acc[v][c] * (1.f / passes) (one fp32 multiply), pred[v] = argmax over c of acc[v][:] (first maximum wins,
 * msk_argmax_c).  probs.p and pred may each be null.  All three: asynchronous on the context stream, no atomics,
 * nothing data-dependent can fail; shape mismatch, mask outside 0..7 and passes < 1 are argument errors.             */
int msk_tta_finish(msk_ctx* ctx, msk_tensor acc, int passes, msk_tensor probs, int32_t* pred);

/* ---- sliding-window inference (core/infer.py sliding_window_inference) ------ */
/* Crop patches.n windows of patches' extent out of vol [N,D,H,W,Cin] with implicit padding.  origins: HOST array of
 * patches.n x 4 int32 (n, d0, h0, w0), the window's first voxel in VOLUME coordinates (may be negative, the window may run
 * past the end):  patches[b][z][y][x][:] = vol[n][d0+z][h0+y][w0+x][:] where that voxel exists, cval where it does not.  */
int msk_sw_gather(msk_ctx* ctx, msk_tensor vol, msk_tensor patches, const int32_t* origins, float cval);
/* Add logits.n windows of logits [B,rd,rh,rw,C], weighted per voxel, into acc [N,D,H,W,C].  td / th / tw: DEVICE tables of
 * nd x rd, nh x rh, nw x rw floats (one row per window start of that axis; core/infer.py SlidingPlan normalises them per axis,
 * so the weights of all windows over a voxel sum to 1 and no division follows).  origins: HOST array of logits.n x 7 int32
 * (n, d0, h0, w0, id, ih, iw): origin as above and the table row of each axis.  For the windows in order, for every window
 * voxel inside the volume (the padding is skipped) and every channel, in fp32 with one rounding per operation, never an FMA:
 *     w   = (td[id][z] * th[ih][y]) * tw[iw][x]
 *     acc = acc + (w * logit)
 * Both entry points: asynchronous on the context stream (origins is read before the call returns), no atomics, one launch
 * per window so that overlapping windows of one call are added in order; any ld >= c on every tensor (16 bytes per lane
 * where the tensors are dense and row start and row length are whole quads, 4 bytes per lane otherwise); nothing
 * data-dependent can fail.  Argument errors, reported before any launch: a channel mismatch, n outside the batch, a table
 * row outside its table, a window that does not intersect the volume, patches overlapping vol, acc overlapping logits.   */
int msk_sw_accumulate(msk_ctx* ctx, msk_tensor logits, const int32_t* origins, const float* td, int nd, const float* th, int nh,
                      const float* tw, int nw, msk_tensor acc);
/* The two above with mirroring inside the window (nnU-Net's predictor; core/infer.py sliding_window_inference(mirror_axes=...),
 * tests/sliding_mirror_reference.py).  A mask mirrors about the WINDOW, m_a(i) = r_a - 1 - i along every axis a whose bit is set
 * (bit 0 = D, bit 1 = H, bit 2 = W, as msk_flip_axes), r_a the window's extent: the implicit padding is mirrored with the content.
 * msk_sw_gather_mirrored: origins is a HOST array of patches.n x 5 int32 (n, d0, h0, w0, mask), a mask per patch;
 *     patches[b][z][y][x][:] = P[m_D(z)][m_H(y)][m_W(x)][:],  P what msk_sw_gather writes for that origin.
 * msk_sw_accumulate_mirrored: origins is a HOST array of logits.n x 8 int32 (n, d0, h0, w0, id, ih, iw, mask).  For the rows in
 * order, every window voxel (z, y, x) inside the volume (volume frame, tables indexed un-mirrored) and every channel c:
 *     w   = (td[id][z] * th[ih][y]) * tw[iw][x]
 *     ws  = w * scale
 *     acc = acc + (ws * logits[row][m_D(z)][m_H(y)][m_W(x)][c])
 * in fp32 with one rounding per operation, never an FMA.  Consecutive rows whose first seven ints are equal are one window's
 * passes: up to 8 of them are ONE launch that reads and writes the accumulator once and every pass's logits once (K + 2 window
 * tensors instead of the 5 K of msk_flip_axes + msk_sw_accumulate per pass); the adds keep the row order, so the result is bit
 * for bit that of one row per call.  One launch per run, in order, no atomics.  With every mask 0 (and scale == 1) the results
 * are those of msk_sw_gather / msk_sw_accumulate bit for bit.  16 bytes per lane on the accumulator side under the conditions
 * above; a W mirror then takes whole source quads for C == 1, C == 2 and C % 4 == 0 and four 4-byte loads for any other C (the
 * gather: quads for D / H mirrors and for W at C == 1).  Argument errors, before any launch: those of the two above, a mask
 * outside 0..7, a scale that is not finite and positive.                                                                  */
int msk_sw_gather_mirrored(msk_ctx* ctx, msk_tensor vol, msk_tensor patches, const int32_t* origins, float cval);
int msk_sw_accumulate_mirrored(msk_ctx* ctx, msk_tensor logits, const int32_t* origins, const float* td, int nd, const float* th,
                               int nh, const float* tw, int nw, float scale, msk_tensor acc);

/* ---- random patch cropping (transforms.RandomPatchCrop3D) -------------------- */
/* Bytes of workspace msk_patch_select needs for a label volume of `voxels` voxels (in [1, 2^31)) and num_classes in
 * [1, 256]: the class totals and one row of num_classes 32-bit counters per 4096 voxels.  Needs no context and no GPU.  */
int msk_patch_workspace(long voxels, int num_classes, size_t* bytes);
/* Choose n_patches (1..16) patch origins of extent rd x rh x rw in a DEVICE label volume [d,h,w] int32, as
 * tests/patch_reference.py states it.  counts[c] = voxels with label c, 0 <= c < num_classes (other values, 255 or negative,
 * are not counted); present = the classes of `classes` (HOST, n_classes in 0..32 strictly ascending values inside
 * [0, num_classes)) with counts > 0, m of them.  words: HOST array of n_patches x 6 uint32 (force_fg, w_cls, w_rank, w_d, w_h,
 * w_w); every product below is an exact unsigned 64-bit one.  With force_fg != 0 and m > 0: cls = present[(w_cls * m) >> 32],
 * r = (w_rank * counts[cls]) >> 32, the centre is the r-th voxel of class cls in raster order, and per axis
 * origin = -((roi - dim) / 2) if dim <= roi, else min(max(centre - roi / 2, 0), dim - roi).  Otherwise cls = -1,
 * centre = (-1,-1,-1) and per axis origin = -((roi - dim) / 2) if dim <= roi, else (w_axis * (dim - roi + 1)) >> 32.
 * sel (DEVICE): n_patches records of 8 int32: d0, h0, w0, cls, cz, cy, cx, 0.  counts (DEVICE, num_classes int32) may be
 * null.  workspace (DEVICE): msk_patch_workspace bytes, 4-byte aligned; its contents mean nothing to the caller.  The label is
 * read once (16 bytes per lane where it is 16-byte aligned), plus one 16 KiB chunk of it per foreground patch; a call in which
 * no patch has force_fg set (or n_classes == 0) and counts is null does not read it at all.                                   */
int msk_patch_select(msk_ctx* ctx, const int32_t* label, int d, int h, int w, int num_classes, const int32_t* classes,
                     int n_classes, int rd, int rh, int rw, const uint32_t* words, int n_patches, void* workspace,
                     int32_t* sel, int32_t* counts);
/* dst [rd,rh,rw] = the patch of src [d,h,w] (4-byte elements, float32 or int32, copied as bits) whose origin is the first
 * three words of ONE sel record, read on the device: dst[z][y][x] = src[d0+z][h0+y][w0+x] where that voxel exists, pad_bits
 * where it does not.  16-byte stores where rw % 4 == 0, 16-byte loads where also w % 4 == 0 and w0 % 4 == 0.
 * All three: integer arithmetic only, integer atomics for the totals only (results do not depend on scheduling); select and
 * crop run asynchronously on the context stream, read their host arrays before they return, synchronise and download
 * nothing, and nothing data-dependent can fail.  Argument errors, reported before any launch: null pointers, extents < 1,
 * 2^31 voxels or more (volume or patch), num_classes outside 1..256, n_classes outside 0..32, a class that is not ascending
 * or outside [0, num_classes), n_patches outside 1..16, dst overlapping src.                                                */
int msk_patch_crop(msk_ctx* ctx, const void* src, int d, int h, int w, const int32_t* sel, void* dst, int rd, int rh, int rw,
                   uint32_t pad_bits);

/* ---- rotated and scaled patch cropping (transforms.RandomAffinePatchCrop3D) ---- */
/* out_img [rd,rh,rw] (and out_label) = the patch of img [d,h,w] float32 (and label, int32) whose sampling grid is built around
 * the centre of ONE sel record of msk_patch_select (DEVICE; its first three words d0, h0, w0 are read on the device), turned
 * and scaled by matrix (HOST, 9 floats, row-major: source axis x patch axis; read before the call returns), as
 * tests/affine_reference.py states it.  For the output voxel (z, y, x), o = (z - rd/2, y - rh/2, x - rw/2), per source axis a:
 *     p_a = ((M[a][0]*o_z + M[a][1]*o_y) + M[a][2]*o_x) + (float)(origin_a + roi_a/2)
 * image: f = floor(p), t = p - f, the eight corners f + {0,1}^3 -- a corner outside the volume has the value pad and is not
 * loaded (scipy's mode='grid-constant') -- and lerp(a, b, t) = a + t*(b - a) along w, then h, then d; label: the voxel at
 * floor(p + 0.5f), label_pad outside the volume.  Every float operation is rounded on its own (no FMA), so the result equals
 * the numpy statement bit for bit; with the identity matrix it equals msk_patch_crop (for data without negative zeros).
 * label and out_label are both null or both set; image and label share the coordinates.  One launch on the context stream, a
 * thread per output voxel (option "affine_map"), no atomics, no synchronisation, no download; nothing data-dependent can fail.
 * Argument errors, reported before any launch: null img, sel, matrix or out_img; only one of label and out_label set;
 * misaligned pointers (4 bytes); extents < 1 or > 8192 per axis (volume or patch); 2^31 voxels or more (volume or patch); a
 * matrix entry that is not finite or whose magnitude exceeds 4 (with the extent limit this bounds |p| below 2^17, so every
 * float -> int conversion is defined); outputs overlapping img, label, sel or each other.                                   */
int msk_affine_patch(msk_ctx* ctx, const float* img, const int32_t* label, int d, int h, int w, const int32_t* sel,
                     const float* matrix, float* out_img, int32_t* out_label, int rd, int rh, int rw, float pad,
                     int32_t label_pad);
/* Elastic deformation of that sampling grid (replaces batchgenerators' elastic_deform_coordinates, the third part of its
 * SpatialTransform, and MONAI's Rand3DElastic; not in the reference), as tests/elastic_reference.py states it.
 *
 * msk_elastic_field: field (DEVICE, float32 [3][rd][rh][rw]) = alpha * (uniform noise smoothed by a Gaussian).  With
 * n = rd*rh*rw and key = splitmix64(seed), component a at patch voxel v = (z*rh + y)*rw + x starts as
 *     u = (float)(splitmix64(key + a*n + v) >> 40) * 2^-23 - 1        (exact, in [-1, 1))
 * and is filtered along w, then h, then d with the HOST taps (2r+1 floats, preprocess.gauss_taps) and zeros outside the patch
 * (scipy's mode='constant'): acc = taps[0]*x[i-r], then acc = acc + taps[k]*x[i-r+k] for k = 1..2r -- all 2r+1 terms, an operand
 * outside the line is +0.0 -- and finally multiplied by alpha; every multiply and add is a float32 operation rounded on its own.
 * A component whose bit is clear in axes_mask (bit a = source axis a) is +0.0 everywhere; the others do not depend on the mask.
 * scratch (DEVICE) has the size of field.  The noise is generated inside the first pass, no noise buffer exists.  Up to three
 * launches and two clears on the context stream; no atomics, no synchronisation, no download; two calls give the same bits.
 * Argument errors, reported before any launch: null pointers; r outside [2, 64]; alpha not finite or outside [0, 4096];
 * axes_mask outside [0, 7]; extents < 1 or > 8192; 3*n >= 2^31; misaligned pointers (4 bytes); field overlapping scratch; a
 * tap that is not finite or outside [0, 1].
 *
 * msk_affine_patch_elastic: msk_affine_patch whose offsets are displaced before the matrix (batchgenerators' order: the
 * zero-centred mesh is deformed, then rotated and scaled, then moved to the centre):
 *     e_a = o_a + field[a][z][y][x]                                    (one float32 add per axis)
 *     p_a = ((M[a][0]*e_z + M[a][1]*e_y) + M[a][2]*e_x) + (float)(origin_a + roi_a/2)
 * and everything from p on as msk_affine_patch; a field of +0.0 gives msk_affine_patch's bits.  With msk_elastic_field's
 * |field| <= 4096 this bounds |p| below 2^18; whatever the field holds, every index is clamped into the volume before it is
 * used.  Argument errors: those of msk_affine_patch, and a null or misaligned field, 3*rd*rh*rw >= 2^31, an output overlapping
 * field.                                                                                                                   */
int msk_elastic_field(msk_ctx* ctx, uint64_t seed, int rd, int rh, int rw, const float* taps, int r, float alpha, int axes_mask,
                      float* field, float* scratch);
int msk_affine_patch_elastic(msk_ctx* ctx, const float* img, const int32_t* label, int d, int h, int w, const int32_t* sel,
                             const float* matrix, const float* field, float* out_img, int32_t* out_label, int rd, int rh, int rw,
                             float pad, int32_t label_pad);

/* ---- intensity augmentation (transforms.RandomGaussianNoise3D / RandomGaussianBlur3D / RandomBrightness3D /
 *      RandomContrast3D / RandomGamma3D; no reference call site: the reference has geometric augmentation only) ---- */
#define MSK_INTENSITY_NOISE 0
#define MSK_INTENSITY_SCALE 1
#define MSK_INTENSITY_CONTRAST 2
#define MSK_INTENSITY_GAMMA 3
#define MSK_INTENSITY_RESTORE 4
/* Bytes of workspace msk_intensity_stats needs for a volume of n voxels (in [1, 2^31)): 24 bytes per chunk of 4096 voxels.
 * Needs no context and no GPU.                                                                                               */
int msk_intensity_stats_workspace(long n, size_t* bytes);
/* stats (DEVICE, 4 doubles, 8-byte aligned) = {min, max, sum, sumsq} of the n float32 of x (DEVICE, 4-byte aligned; finite),
 * as tests/intensity_reference.py states it: min and max exact; sum and sumsq in float64 in a FIXED order -- chunk c covers
 * the voxels [4096c, 4096(c+1)), lane l of 256 adds x[l], x[l+256], ..., x[l+3840] in ascending order (elements past n add
 * +0.0), sumsq adds the exact (double)x * (double)x, the 256 lane values are combined by the tree v[l] += v[l+s], s = 128,
 * 64, ..., 1, and the chunk values are reduced by the same scheme (lane l adds P[l], P[l+256], ..., then the tree).  Two
 * launches on the context stream, no atomics, no synchronisation, no download.  workspace (DEVICE): 8-byte aligned,
 * msk_intensity_stats_workspace bytes; its contents mean nothing to the caller.                                              */
int msk_intensity_stats(msk_ctx* ctx, const float* x, long n, void* workspace, double* stats);
/* One streaming pass y[i] = f(x[i]) over n float32 (DEVICE, 4-byte aligned; 16 bytes per lane where both are 16-byte aligned;
 * y == x is allowed, any other overlap is an error).  params: HOST array of 4 floats, read before the call returns.  stats_a /
 * stats_b: DEVICE records of msk_intensity_stats, read on the device (nothing synchronises); a mode that does not use one
 * accepts null.  Every float operation is rounded on its own (no FMA).  mode:
 *   NOISE     y = x + p0 * z_i;  k = splitmix64(seed), h = splitmix64(k + i), u1 = ((h >> 40) + 1) * 2^-24,
 *             u2 = ((h >> 8) & 0xFFFFFF) * 2^-24, z = sqrtf(-2 logf(u1)) * cosf(2 pi u2)
 *   SCALE     y = x * p0
 *   CONTRAST  (stats_a) m = (float)(sum_a / n);  y = ((x - m) * p0) + m, clamped to [(float)min_a, (float)max_a] if p1 != 0
 *   GAMMA     (stats_a) s = p1 != 0 ? -1 : 1;  (mn, mx) = s > 0 ? (min_a, max_a) : (-max_a, -min_a);  rg = mx - mn;
 *             y = s * (powf((s * x - mn) / (rg + 1e-7f), p0) * rg + mn)
 *   RESTORE   (stats_a of the volume before, stats_b of x) mean = sum / n, sd = sqrt(max(sumsq / n - mean * mean, 0)) in
 *             float64, rounded to float32;  y = (x - mean_b) / (sd_b + 1e-8f) * sd_a + mean_a                                 */
int msk_intensity_apply(msk_ctx* ctx, const float* x, float* y, long n, int mode, const float* params, const double* stats_a,
                        const double* stats_b, uint64_t seed);
/* y [d,h,w] = x blurred along d, then h, then w with HOST taps of 2r+1 floats per axis (r in 0..8; r == 0 skips the axis, all
 * three 0 copy) and scipy's mode='reflect': per pass out[i] = sum over k = -r..r ascending of w[k] * in[reflect(i + k)], a
 * float32 multiply then a float32 add, starting from the first product;  reflect(i) = m < n ? m : 2n-1-m, m = i mod 2n >= 0
 * (any extent >= 1).  y must not overlap x; tmp (DEVICE, d*h*w floats, overlapping neither) is needed when two or three axes
 * are blurred.  Up to three launches on the context stream, no atomics.  Argument errors of all four, reported before any
 * launch: null or misaligned pointers, n or d*h*w outside [1, 2^31), an unknown mode, a missing record, r outside 0..8,
 * overlapping buffers.                                                                                                       */
int msk_gauss_blur3d(msk_ctx* ctx, const float* x, float* y, int d, int h, int w, const float* taps_d, int r_d,
                     const float* taps_h, int r_h, const float* taps_w, int r_w, float* tmp);

/* ---- loss ------------------------------------------------------------------ */
/* losses/loss_utils.py:31-40 class_weights: w_c = sum(1-softmax_c)/sum(softmax_c) */
int msk_class_weights(msk_ctx* ctx, msk_tensor logits, float* weights);
/* Fused CrossEntropyLoss + DiceLoss forward (losses/cross_entropy_loss.py:47-87,
 * losses/dice_loss.py:76-102).  out[0]=CE, out[1]=dice loss, out[2..2+C)=per-channel
 * dice; stats (device, 3*C+2 doubles) keeps {I_c, S_c, T_c, ce_num, ce_den} for bwd. */
int msk_loss_fwd(msk_ctx* ctx, msk_tensor logits, const int32_t* labels, const float* weights,
                 int ignore_index, float* out, double* stats);
/* dlogits = coef_ce * dCE/dz + coef_dice * dDice/dz */
int msk_loss_bwd(msk_ctx* ctx, msk_tensor logits, const int32_t* labels, const float* weights,
                 int ignore_index, const double* stats, float coef_ce, float coef_dice,
                 msk_tensor dlogits);

/* DiceLoss(sigmoid_norm=False) and DiceLoss(weight=...) (losses/dice_loss.py:36-43,68-69): dice_softmax != 0
 * normalises the dice term's probabilities with softmax over the classes instead of the sigmoid; dice_weight
 * (device, [C], or NULL) multiplies each class's intersection.  The CE term is unchanged. */
int msk_loss_fwd_ex(msk_ctx* ctx, msk_tensor logits, const int32_t* labels, const float* weights,
                    int ignore_index, int dice_softmax, const float* dice_weight, float* out, double* stats);
int msk_loss_bwd_ex(msk_ctx* ctx, msk_tensor logits, const int32_t* labels, const float* weights,
                    int ignore_index, int dice_softmax, const float* dice_weight, const double* stats,
                    float coef_ce, float coef_dice, msk_tensor dlogits);

/* BCELoss (losses/binary_cross_entropy_loss.py:84-172): binary_cross_entropy_with_logits against y = the label value
 * (C == 1) or one_hot(label, C) (C > 1; a label outside [0, C) gives an all-zero row), masked by label != ignore_index,
 * loss = mean(l * mask) / (mean(mask) + 1e-10) with mask [N,1,D,H,W].  weight_mode 0 = None, 1 = 'dynamic' (:131-139);
 * pos_weight_mode 0 = None, 1 = pos_weight, 2 = 'dynamic' (:142-148).  The pos / neg / mask counts are exact.
 * out[0] = loss; stats (device, 8 doubles) = {w_pos, w_neg, pw, scale, sum(l mask), sum(mask), pos, neg} for bwd. */
int msk_bce_fwd(msk_ctx* ctx, msk_tensor logits, const int32_t* labels, int ignore_index, int weight_mode,
                int pos_weight_mode, float pos_weight, float* out, double* stats);
/* dlogits (+)= coef * dloss/dlogits (accumulate != 0 adds: BCE after CE / Dice on the same logits); the weights
 * carry no gradient (:161-162 stop_gradient) */
int msk_bce_bwd(msk_ctx* ctx, msk_tensor logits, const int32_t* labels, int ignore_index, const double* stats,
                float coef, int accumulate, msk_tensor dlogits);

/* Region losses under a mask (SoftDiceLoss, TverskyLoss, FocalLoss, DiceCELoss; tests/region_reference.py is the statement):
 * L = coef_r L_r + coef_f L_f, the coefficients given to the backward call.  Per voxel m = (label != ignore_index),
 * t_c = (label == c) (C == 1: label == 1; a label outside [0, C) gives an all-zero row), p = softmax over the classes
 * (activation 0, C >= 2) or sigmoid (activation 1).  Per group g (the batch when batch_dice != 0, else each sample; G groups)
 * and class c: TP = sum m p t, SP = sum m p^q (q = 2 when squared_pred != 0, else 1), ST = sum m t.
 *   mode 0 (Dice):    score = (2 TP + smooth) / max(SP + ST + smooth, 1e-8)
 *   mode 1 (Tversky): score = (TP + smooth) / (TP + alpha (SP - TP) + beta (ST - TP) + smooth)     (q = 1 only)
 *   L_r = 1 - mean of score over the groups and the scored classes K (all classes, or 1 .. C-1 when do_bg == 0 and C > 1)
 *   dL_r/dp = m (A t + B q p^(q-1)),  A = -(dscore/dTP) / (G |K|),  B = -(dscore/dSP) / (G |K|),  both 0 outside K
 *   L_f (focal_on != 0, softmax only) = sum v w_y (1 - u)^gamma (-log u) / sum v w_y over the voxels v with m = 1 and
 *   0 <= label < C, u = p_label, w = weight (device, [C]) or ones when NULL; 0 when the denominator is 0.  gamma = 0 is plain
 *   cross entropy; gamma must be 0 or >= 1.  The logits are used as given.
 * out (device, 2 + C floats) = {L_f, L_r, mean over the groups of score[., c] for every class c}.
 * stats (device, 5 G C + 2 doubles) = TP[G][C], SP[G][C], ST[G][C], A[G][C], B[G][C], f_num, f_den.
 * Nothing is downloaded and nothing synchronises.  With several ranks the sums are those of the calling rank. */
int msk_region_loss_fwd(msk_ctx* ctx, msk_tensor logits, const int32_t* labels, int ignore_index, int activation,
                        int squared_pred, int batch_dice, int do_bg, int mode, float smooth, float alpha, float beta,
                        int focal_on, float gamma, const float* weight, float* out, double* stats);
/* dlogits (+)= coef_f dL_f/dlogits + coef_r dL_r/dlogits from the stats of the forward call with the same settings
 * (accumulate != 0 adds: a region loss after CE / Dice on the same logits).  dlogits has the logits' shape. */
int msk_region_loss_bwd(msk_ctx* ctx, msk_tensor logits, const int32_t* labels, int ignore_index, int activation,
                        int squared_pred, int batch_dice, int do_bg, int mode, float smooth, float alpha, float beta,
                        int focal_on, float gamma, const float* weight, const double* stats, float coef_f, float coef_r,
                        int accumulate, msk_tensor dlogits);

/* ---- region-based training: sigmoid Dice + BCE over label regions (DiceBCERegionLoss: nnU-Net's DC_and_BCE_loss and its
 *      regions_class_order; tests/mlabel_reference.py is the statement) ---- */
/* The R = logits.c channels (1 <= R <= 32) are overlapping REGIONS of the label map.  The label stays one int32 per voxel;
 * table (DEVICE, table_len uint32, 1 <= table_len <= 256) maps a label value v to the bit mask of the regions it belongs to.
 * Per voxel m = (label != ignore_index), t_r = bit r of table[label] when 0 <= label < table_len, otherwise 0 (a label outside
 * the table that is not ignored gives an all-zero row), p_r = sigmoid(z_r) in the overflow-free form (exp(-|z|)).  Per group g
 * (the batch when batch_dice != 0, else each sample; G groups) and region r: TP = sum m p t, SP = sum m p^q (q = 2 when
 * squared_pred != 0, else 1), ST = sum m t.
 *   score  = (2 TP + smooth) / den,  den = max(SP + ST + smooth, 1e-8)
 *   L_dice = 1 - mean of score over the groups and ALL regions (there is no do_bg)
 *   L_bce  = sum m sum_r (max(z, 0) - z t + log1p(exp(-|z|))) / (R sum m), 0 when no voxel is valid
 *   dL/dz  = coef_bce m (p - t) / (R sum m) + coef_dice m (A t + B q p^(q-1)) p (1 - p)
 *   A = -2 / (G R den),  B = (2 TP + smooth) / (G R den^2) where SP + ST + smooth > 1e-8, otherwise 0
 * out (device, 2 + R floats) = {L_bce, L_dice, mean over the groups of score[., r] for every region r}.
 * stats (device, 5 G R + 2 doubles) = TP[G][R], SP[G][R], ST[G][R], A[G][R], B[G][R], the BCE sum, sum m.
 * Two launches; no float atomics, two calls give the same bits; nothing is downloaded and nothing synchronises.  With several
 * ranks the sums are those of the calling rank. */
int msk_mlabel_loss_fwd(msk_ctx* ctx, msk_tensor logits, const int32_t* labels, int ignore_index, const uint32_t* table,
                        int table_len, int squared_pred, int batch_dice, float smooth, float* out, double* stats);
/* dlogits (+)= the gradient above from the stats of the forward call with the same settings (accumulate != 0 adds).  One
 * launch.  Argument errors of both, reported before any launch: R outside 1..32, table_len outside 1..256, null or misaligned
 * pointers, a dlogits of another shape or overlapping the logits, a voxel count at or above 2^31, smooth < 0. */
int msk_mlabel_loss_bwd(msk_ctx* ctx, msk_tensor logits, const int32_t* labels, int ignore_index, const uint32_t* table,
                        int table_len, int squared_pred, int batch_dice, float smooth, const double* stats, float coef_bce,
                        float coef_dice, int accumulate, msk_tensor dlogits);
/* out [N,D,H,W] int32 = 0, then for r = 0 .. R-1 in order: out = class_order[r] where logit z_r > 0 (the last region that
 * fires wins: nnU-Net's loop over regions_class_order; the comparison is on the logit, a NaN does not fire).  class_order: HOST,
 * R = logits.c values, read during the call (it travels by value in the kernel arguments).  One launch; the same argument
 * errors. */
int msk_regions_to_label(msk_ctx* ctx, msk_tensor logits, const int32_t* class_order, int32_t* out);

/* ---- top-k selection and top-k cross entropy (TopKLoss, DiceTopKLoss: nnU-Net's TopKLoss / DC_and_topk_loss;
 *      tests/topk_reference.py is the statement) ---- */
/* Bytes of workspace for n values (in [1, 2^31)): the n floats of per-voxel loss, three 2048-bin histograms, 8 bytes per chunk of
 * 4096 values.  Needs no context and no GPU.                                                                                   */
int msk_topk_workspace(long n, size_t* bytes);
/* record (DEVICE, 8 doubles, 8-byte aligned) = {T, K, n_gt, n_eq, S_gt, r, tie_w, S} of the K = k largest of the n float32 of x
 * (DEVICE, 4-byte aligned, not modified).  Values are ordered by the sortable key of their bit pattern (sign bit set: all bits
 * flipped, otherwise the sign bit set: -0.0 < +0.0, a NaN with a clear sign bit above +inf).  T = the value with the K-th
 * largest key, n_gt / n_eq = the keys above / equal to it, S_gt = the float64 sum of the values above it in the FIXED order of
 * msk_intensity_stats (chunks of 4096, 256 lanes, the tree, then the chunk values by the same scheme; a value that is not above T
 * adds +0.0), r = K - n_gt, tie_w = r / n_eq, S = S_gt + r T (a product, then a sum).  k == 0: all zeros.  Every field is exact.
 * One memset and five launches on the context stream: three histogram passes over digits of 11, 11 and 10 bits (integer LDS
 * and global atomics), the ordered sum, the finish.  No float atomics, no synchronisation, no download.  workspace (DEVICE): 16-byte aligned,
 * msk_topk_workspace(n) bytes, overlapping neither x nor record; its contents mean nothing to the caller.                       */
int msk_topk_select(msk_ctx* ctx, const float* x, long n, long k, void* workspace, double* record);
/* Top-k cross entropy of logits [N,D,H,W,C] (ld >= C, 2 <= C <= 64, V = N D H W < 2^31) against int32 labels.  A voxel is valid
 * when its label is in [0, C) and is not ignore_index.  l_i = w_y (logf(sum_c expf(z_c - m)) - (z_y - m)), m the row maximum,
 * w = weights (DEVICE, [C], all >= 0) or ones when NULL; an invalid voxel gets the sentinel -1.  K = floor((double)n_valid *
 * (double)k_percent / 100), at least 1 when n_valid > 0, evaluated on the device; record = the msk_topk_select record of the l_i
 * for that K; out (DEVICE, 2 + C floats) = {S / K (0 when n_valid == 0), 0, ...}.  The l_i stay in the workspace (its first V
 * floats) for the backward call.  One memset and five launches; nothing is downloaded and nothing synchronises.  With several
 * ranks the selection is that of the calling rank.                                                                              */
int msk_topk_ce_fwd(msk_ctx* ctx, msk_tensor logits, const int32_t* labels, int ignore_index, const float* weights,
                    float k_percent, void* workspace, float* out, double* record);
/* dz (+)= coef u_i w_y (softmax(z_i) - onehot(y_i)) / K from the workspace and the record of the forward call: u_i = 1 for
 * l_i above T, tie_w for l_i at T (tied voxels share the remaining weight: a subgradient with the loss's value that needs no
 * raster order), 0 below and at invalid voxels (exact zeros).  Membership compares the stored l_i, so it is the forward's bit
 * for bit.  accumulate != 0 adds into dz.  One launch.  Argument errors of all four, reported before any launch: null or
 * misaligned pointers, n or V outside [1, 2^31), k outside [0, n], k_percent outside (0, 100], C outside 2..64, a dz of another
 * shape, a workspace that overlaps an operand.                                                                                  */
int msk_topk_ce_bwd(msk_ctx* ctx, msk_tensor logits, const int32_t* labels, int ignore_index, const float* weights,
                    const void* workspace, const double* record, float coef, int accumulate, msk_tensor dz);

/* ---- Lovasz-Softmax loss on an exact key-index radix sort (LovaszSoftmaxLoss, DiceLovaszLoss: Berman, Triki, Blaschko, CVPR
 *      2018, PaddleSeg's LovaszSoftmaxLoss; the reference has no such loss, so every entry cites tests/lovasz_reference.py, the
 *      statement) ---- */
/* Bytes of workspace for `groups` groups of `voxels` voxels each (in [1, 2^31)) and `classes` classes (2 .. 64, groups x classes
 * <= 65535): four planes of S = voxels rounded up to 64 words per (group, class), the histograms of a digit pass, 16 bytes per
 * chunk of 4096 keys and plane.  Needs no context and no GPU.                                                                   */
int msk_lovasz_workspace(long voxels, int classes, int groups, size_t* bytes);
/* Lovasz-Softmax of logits [N,D,H,W,C] (ld >= C, 2 <= C <= 64) against int32 labels.  A group is the whole batch, or one sample
 * when per_image != 0; its voxels are taken in raster order.  A voxel is valid when its label is in [0, C) and is not
 * ignore_index; every other voxel takes no part.  Per (group g, class c) the plane p = g C + c: e_v = |[y_v == c] - p_vc| with p
 * the float32 softmax (row maximum, expf, the sum in ascending class order, one division), sorted in descending order, ties in
 * ascending voxel order; with G the plane's foreground voxels and cf_i those at sorted positions <= i,
 * J_i = 1 - (G - cf_i) / (G + i + 1 - cf_i), g_i = J_i - J_{i-1} (J_{-1} = 0) in float64 from exact integers, and
 * L = sum_i float64(e_(i)) g_i in the FIXED order of msk_intensity_stats over the sorted positions.  A class counts in its group
 * when G > 0 (class_mode 0), always (1: a class with G = 0 has g_0 = 1 and nothing else), or when G > 0 and its bit is set in
 * class_mask (2).  loss = the mean over the groups of the mean of L over the group's counted classes (0 for a group without one).
 * out (DEVICE, 2 + C floats) = {loss, counted (group, class) pairs, per class the mean L over the groups that count it}.
 * stats (DEVICE, 4 groups C + 2 doubles, 8-byte aligned) = per plane {n_valid, G, L, scale = 1 / (groups x counted classes of
 * the group), 0 for a class that does not count}, then {loss, pairs}; every field is exact and reproducible.  workspace (DEVICE,
 * 16-byte aligned, at least msk_lovasz_workspace(voxels of a group, C, groups) bytes, overlapping no operand) holds afterwards,
 * in planes of S words each starting on a 256-byte boundary: the sorted keys of all planes (bits 0-29: 0x3f800000 - the bits of
 * e, ascending; bit 31: [y == c]; 0x3fffffff: a voxel that takes no part, behind all valid ones), then their voxel indices inside
 * the group (the permutation), then the float32 planes dL/de_v = float32(g_rank(v) scale), 0 at a voxel that takes no part.
 * 22 launches on the context stream: the pack, four digit passes of 8, 8, 8 and 6 bits (histogram, two scan kernels, stable
 * scatter of key and index), the foreground prefix, the sums, the finish.  Integer atomics in LDS histograms only, no float
 * atomics, no synchronisation, no download.  With several ranks the sort is that of the calling rank.                            */
int msk_lovasz_fwd(msk_ctx* ctx, msk_tensor logits, const int32_t* labels, int ignore_index, int class_mode,
                   unsigned long long class_mask, int per_image, void* workspace, size_t workspace_bytes, float* out,
                   double* stats);
/* dz_k (+)= coef p_k (s_k ge_k - sum_c s_c ge_c p_c) with ge = the dL/de planes the forward call left in the workspace, p the
 * softmax recomputed, s_c = -1 where y == c and +1 elsewhere; evaluated as p_k ((a_k - a_m) + sum_c p_c (a_m - a_c)) with
 * a = s ge and m the class of the largest probability, which does not cancel where the softmax is nearly one-hot.  A voxel that
 * takes no part gets zeros; when accumulate != 0 adds into dz its value stays (a lane's own form skips it, the LDS-tile forms add
 * +0.0 to it, which turns a stored -0.0 into +0.0).  stats is the record of the forward call (it travels with the workspace; the
 * pass reads the planes only).  One launch.  Argument errors of all three, reported before any launch: null or misaligned
 * pointers, C outside 2..64, a group of 2^31 voxels or more, a workspace that is too small or overlaps an operand, a class_mode
 * outside 0..2, a class_mask that is empty or names a class outside [0, C), a dz of another shape.                               */
int msk_lovasz_bwd(msk_ctx* ctx, msk_tensor logits, const int32_t* labels, int ignore_index, int per_image,
                   const void* workspace, size_t workspace_bytes, const double* stats, float coef, int accumulate, msk_tensor dz);

/* ---- boundary loss on signed distance maps built on the device (BoundaryLoss, DiceBoundaryLoss: Kervadec et al., MIDL 2019,
 *      the BDLoss / DC_and_BD_loss of the nnU-Net loss collections; the reference has no such loss, so every entry cites
 *      tests/boundary_reference.py, the statement) ---- */
/* Bytes of workspace for one volume of d x h x w voxels (every extent in 1 .. MSK_EDT_MAX_EXTENT): its two float64 distance
 * fields, each rounded up to 256 bytes.  Needs no context and no GPU.  (tests/boundary_reference.py: signed_distance)          */
int msk_sdf_workspace(int d, int h, int w, size_t* bytes);
/* Signed distance maps of the int32 labels [n][d][h][w] (DEVICE, not modified) for the classes whose bit is set in class_mask.
 * phi (DEVICE, 16-byte aligned) is class-planar: plane (s * |S| + j) holds the V = d h w floats of sample s and the j-th set bit
 * c.  With pos = (label == c) (everything else is outside, 255 and labels beyond the class range included),
 *   d_out = sqrt(msk_edt3d's dist2 to the features {== c}),  d_in = sqrt(dist2 to the features {!= c}),   both float64,
 *   phi = d_out outside the class, 1 - d_in inside it (a voxel with d_in = 1 gets +0.0), 0 where the squared distance is +inf
 *   (the class is absent from the volume or fills it),   rounded once to float32.
 * Bit for bit tests/boundary_reference.py: signed_distance, which equals Kervadec's one_hot2dist wherever the class is present
 * and does not fill the volume.  Per (sample, class) two exact transforms (the passes of msk_edt3d; the complement comes from a
 * complemented x pass, no mask volume is written) and one compose pass: seven launches, in the two fields of the workspace
 * (DEVICE, 16-byte aligned, workspace_bytes >= msk_sdf_workspace(d, h, w)), which are reused from one to the next.  spacing
 * (HOST, nullable = 1, 1, 1): sz, sy, sx, in msk_edt3d's range; the constant 1 is Kervadec's whatever the spacing.  No atomics,
 * nothing is downloaded, nothing synchronises.  n d h w < 2^31.                                                                */
int msk_label_sdf(msk_ctx* ctx, const int32_t* labels, int n, int d, int h, int w, uint64_t class_mask,
                  const double* spacing /* HOST, nullable */, void* workspace, size_t workspace_bytes, float* phi);
/* Boundary loss of logits [N,D,H,W,C] (ld >= C, 2 <= C <= 64) against the maps phi of msk_label_sdf for the same class_mask S.
 * A voxel is valid when its label is in [0, C) and is not ignore_index (the top-k loss's rule); p = softmax(z);
 *   t_c(v) = p_c(v) phi_c(v) for c in S at valid v, else 0;   L = sum t / (n_valid |S|),   A = sum |t| / (n_valid |S|),
 *   L_c = sum_v t_c(v) / n_valid.
 * out (DEVICE, 2 + C floats) = {L, A, L_c for every class (0 outside S)}; stats (DEVICE, 3 + C doubles) = {n_valid, sum t,
 * sum |t|, sum t_c per class}; n_valid == 0: L = A = L_c = 0.  fp32 per-thread sums, one record per workgroup, merged by one
 * workgroup in float64 in a fixed order: no float atomics, two calls give the same bits.  Two launches.
 * (tests/boundary_reference.py: boundary_loss)                                                                                 */
int msk_boundary_loss_fwd(msk_ctx* ctx, msk_tensor logits, const int32_t* labels, int ignore_index, uint64_t class_mask,
                          const float* phi, float* out, double* stats);
/* dlogits_k(v) (+)= coef p_k(v) ([k in S] phi_k(v) - sum_{c in S} t_c(v)) / (n_valid |S|) at the valid voxels (classes outside S
 * do get a gradient), n_valid read from the forward's stats on the device.  An invalid voxel gets exactly 0, or is left as it is
 * when accumulate != 0.  One launch.  (tests/boundary_reference.py: boundary_loss)
 * Argument errors of all four, reported before any launch: C outside 2..64, an empty class_mask or one with a bit >= C, an extent
 * outside 1..MSK_EDT_MAX_EXTENT, N V >= 2^31, a null pointer, phi or the workspace not 16-byte aligned, a workspace that is too
 * small, spacing outside msk_edt3d's range, dlogits overlapping logits or phi, a dlogits of another shape.                      */
int msk_boundary_loss_bwd(msk_ctx* ctx, msk_tensor logits, const int32_t* labels, int ignore_index, uint64_t class_mask,
                          const float* phi, const double* stats, float coef, int accumulate, msk_tensor dlogits);

/* ---- foreground statistics, percentile clipping, z-scoring and the non-zero bounding box (nnU-Net's crop_to_nonzero,
 *      CTNormalization, ZScoreNormalization; preprocess.fg_stats_device / clip_zscore_device / nonzero_bbox_device;
 *      tests/normalize_reference.py is the statement) ---- */
#define MSK_MASK_ALL 0      /* every voxel is valid */
#define MSK_MASK_NONZERO 1  /* x != 0 (so -0.0 is outside); nnU-Net's hole-filled mask: msk_fill_holes3d, then MSK_MASK_LABEL */
#define MSK_MASK_LABEL 2    /* mask > 0, mask an int32 buffer of n words */
#define MSK_NORM_CLIP 1     /* flags of msk_clip_zscore */
#define MSK_NORM_ZSCORE 2
#define MSK_NORM_MASK_OUT 4
/* Bytes of workspace msk_fg_stats needs for n values (in [1, 2^31)): five 2048-bin histograms and 32 bytes per chunk of 4096
 * values.  Needs no context and no GPU.                                                                                       */
int msk_fg_stats_workspace(long n, size_t* bytes);
/* record (DEVICE, 16 doubles, 8-byte aligned) = {n_valid, min, max, sum, sumsq, mean, std, p_lo, p_hi, a_lo, b_lo, g_lo, a_hi,
 * b_hi, g_hi, 0} of the valid voxels among the n float32 of x (DEVICE, 4-byte aligned, finite, not modified); mask (DEVICE, n
 * int32, not modified) is read with MSK_MASK_LABEL only and may be NULL otherwise.  Values are ordered by msk_topk_select's
 * sortable key; s = the valid values in ascending order.  n_valid, min = s[0], max = s[n_valid-1] are exact; sum and sumsq are
 * float64 sums in the FIXED order of msk_intensity_stats over the full raster, an invalid voxel adding +0.0; mean = sum /
 * n_valid, std = sqrt(max(sumsq / n_valid - mean * mean, 0)).  Percentiles (numpy's default method): h = (n_valid - 1) *
 * (q / 100.0), i = floor(h), g = h - i, a = s[i], b = s[min(i + 1, n_valid - 1)], d = b - a, p = g >= 0.5 ? b - d * (1 - g) :
 * a + d * g; K = n_valid - i, h, i and g are evaluated on the device.  Every operation is a float64 operation rounded on its
 * own; every field is exact.  n_valid == 0: all zeros.  One memset and five launches on the context stream: three histogram
 * passes that carry both order statistics (integer LDS and global atomics), the ordered sums with the minimum above each a
 * riding along, the finish.  No float atomics, no synchronisation, no download.  workspace (DEVICE): 16-byte aligned,
 * msk_fg_stats_workspace(n) bytes, overlapping neither x, mask nor record; its contents mean nothing to the caller.
 * Non-finite x gives unspecified values but no access outside the buffers.                                                    */
int msk_fg_stats(msk_ctx* ctx, const float* x, const int32_t* mask, long n, int mask_mode, double q_lo, double q_hi,
                 void* workspace, double* record);
/* One streaming pass over n float32 (DEVICE, 4-byte aligned; 16 bytes per lane where x, y and a mask that is read are 16-byte
 * aligned; y == x is allowed, any other overlap is an error).  lo = (float)p_lo, hi = (float)p_hi, m = (float)mean, inv =
 * (float)(1.0 / max(std, 1e-8)) come from record (DEVICE, a msk_fg_stats record, read on the device behind the thread's first
 * loads: nothing synchronises) or, when record is NULL, from host_params (HOST, 4 doubles {lo, hi, mean, std}, read before the
 * call returns); the two give the same bits for the same values.  In float32, every operation rounded on its own:
 * c = x < lo ? lo : x;  c = c > hi ? hi : c (MSK_NORM_CLIP);  y = (c - m) * inv (MSK_NORM_ZSCORE).  With MSK_NORM_MASK_OUT a voxel
 * that is not valid under mask_mode (see msk_fg_stats; mask is read with MSK_MASK_LABEL and MSK_NORM_MASK_OUT only) becomes
 * `outside`; otherwise it is transformed like every other voxel.  One launch.                                                 */
int msk_clip_zscore(msk_ctx* ctx, const float* x, const int32_t* mask, long n, int mask_mode, const double* record,
                    const double* host_params, int flags, float outside, float* y);
/* box (DEVICE, 8 int32, 4-byte aligned) = {d0, h0, w0, d1, h1, w1, count, 0} of the non-zero voxels of a [d, h, w] volume
 * (DEVICE, 4-byte aligned, not modified; dtype 0 = float32: x != 0, a NaN counts; 1 = int32: v != 0): the upper corner is
 * exclusive, all zeros for an empty volume.  Filling holes does not change a bounding box, so this is the box of nnU-Net's filled
 * mask.  One memset, one streaming pass and a one-thread finish on the context stream; a workgroup reduces its six extremes and
 * its count in registers and LDS and, only if it saw a non-zero voxel, adds its count and sends the extremes that still move the
 * record (at most seven integer atomics).  Nothing synchronises.
 * Argument errors of all four, reported before any launch: null pointers, n outside [1, 2^31), extents < 1 or 2^31 voxels and
 * more, q outside [0, 100] or q_lo > q_hi, an unknown mask_mode / dtype / flag, MSK_MASK_LABEL without a mask, a misaligned
 * record or box, a workspace that is misaligned or overlaps an operand (its size is not passed: the caller owes
 * msk_fg_stats_workspace(n) bytes).                                                                                           */
int msk_nonzero_bbox(msk_ctx* ctx, const void* src, int d, int h, int w, int dtype, int32_t* box);

/* ---- optimizer --------------------------------------------------------------- */
/* paddle.optimizer.Momentum(momentum, weight_decay=L2) over one flat arena
 * (cvlibs/config.py:212-214): g += wd*p; v = mu*v + g; p -= lr*v.
 * grad_scale multiplies g first (1/nranks after a sum all-reduce).              */
int msk_sgd_momentum(msk_ctx* ctx, float* param, const float* grad, float* velocity,
                     size_t count, float lr, float momentum, float weight_decay,
                     float grad_scale);

/* The same update for ONE slice of the arena as soon as everything that produces its gradients has been enqueued
 * (core/train.py:139-140: loss.backward(); optimizer.step() -- nothing reads a block's weights between its data gradient and the
 * next forward).  The update and the re-pack of the slice's convolution weights run at the end of the internal weight-gradient
 * stream, behind an event on the calling stream's current tail; the calling stream does not wait.  Opt-in
 * (optimizer.Momentum.enable_eager): parameters change during backward, and the gradients must be final when the call is made
 * (one rank, or after the slice's all-reduce).  msk_sgd_momentum_finish joins: call it where optimizer.step() stands. */
int msk_sgd_momentum_eager(msk_ctx* ctx, float* param, const float* grad, float* velocity,
                           size_t count, float lr, float momentum, float weight_decay,
                           float grad_scale);
int msk_sgd_momentum_finish(msk_ctx* ctx);

/* paddle.optimizer.Adam(beta1, beta2, epsilon, weight_decay=L2) over one flat arena (cvlibs/config.py:214-216):
 * g = grad_scale*grad + wd*p; m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2;
 * p -= lr sqrt(1-beta2_pow)/(1-beta1_pow) * m / (sqrt(v) + epsilon sqrt(1-beta2_pow));
 * beta*_pow = beta*^t of THIS step (t = 1 on the first call); the caller keeps the powers. */
int msk_adam(msk_ctx* ctx, float* param, const float* grad, float* moment1, float* moment2,
             size_t count, float lr, float beta1, float beta2, float epsilon, double beta1_pow,
             double beta2_pow, float weight_decay, float grad_scale);

/* ---- gradient clipping and Nesterov momentum (paddle.nn.ClipGradByGlobalNorm / ClipGradByValue, Momentum(use_nesterov=True):
 *      the reference hands grad_clip and use_nesterov to paddle.optimizer, cvlibs/config.py:217-224;
 *      tests/clip_reference.py is the statement) ---- */
/* Bytes of workspace msk_grad_clip_coef needs for count gradients (in [1, 2^31)): 8 bytes per chunk of 4096.  Needs no context
 * and no GPU.                                                                                                                */
int msk_grad_clip_workspace(size_t count, size_t* bytes);
/* rec (DEVICE, 4 doubles, 8-byte aligned) = {S, norm, coef, 0} of the count float32 of grad (DEVICE, 16-byte aligned: an
 * arena): S = the sum of the exact (double)g * (double)g in float64 in the FIXED order of msk_intensity_stats -- chunk c covers
 * [4096c, 4096(c+1)), lane l of 256 adds its 16 terms in ascending order (elements past count add +0.0), the tree v[l] +=
 * v[l+s], s = 128 .. 1, and the chunk values are reduced by the same scheme;  norm = (double)grad_scale * sqrt(S);  coef =
 * (float)(clip_norm / norm) if norm > clip_norm, else 1 (clip_norm = +inf measures only), stored as a double.  It first joins
 * the internal weight-gradient stream, then makes two launches on the context stream: no atomics, no synchronisation, no
 * download -- the update below reads the record on the device.  workspace (DEVICE): 8-byte aligned, msk_grad_clip_workspace
 * bytes; its contents mean nothing to the caller.  Argument errors, reported before any launch: null or misaligned pointers,
 * count outside [1, 2^31), clip_norm NaN or <= 0.                                                                            */
int msk_grad_clip_coef(msk_ctx* ctx, const float* grad, size_t count, float grad_scale, float clip_norm, void* workspace,
                       double* rec);
/* msk_sgd_momentum with Paddle's order clip, L2 decay, momentum:  gs = grad_scale * (float)clip_rec[2] (one float32 product;
 * clip_rec: DEVICE record of msk_grad_clip_coef, read on the device, or null = 1);  g' = g * gs, clamped to [clip_min,
 * clip_max] unless both are infinite (a NaN stays a NaN);  t = g' + wd*p;  v = mu*v + t;  p -= lr*v, or with nesterov != 0
 * p -= lr*(t + mu*v) (paddle's use_nesterov: param - (grad + velocity_out * mu) * lr).  The fmaf chain per element is
 * msk_sgd_momentum's: with clip_rec null or coef == 1, infinite bounds and nesterov == 0 the results are bitwise its.  One
 * launch over the whole range behind a join of the weight-gradient stream, then the re-pack of the convolution weights.      */
int msk_sgd_momentum_clip(msk_ctx* ctx, float* param, const float* grad, float* velocity, size_t count, float lr,
                          float momentum, float weight_decay, float grad_scale, int nesterov, const double* clip_rec,
                          float clip_min, float clip_max);
/* msk_adam on the same g' (clip_rec, clip_min, clip_max as above); bitwise msk_adam when nothing bites.                       */
int msk_adam_clip(msk_ctx* ctx, float* param, const float* grad, float* moment1, float* moment2, size_t count, float lr,
                  float beta1, float beta2, float epsilon, double beta1_pow, double beta2_pow, float weight_decay,
                  float grad_scale, const double* clip_rec, float clip_min, float clip_max);

/* ---- preprocessing (tools/preprocess_utils) ----------------------------------- */
/* geometry.py:31-69 resample == scipy.ndimage.zoom(order 0|1, grid_mode=False):
 * align-corner coordinate map; order 0 = floor(c+0.5), order 1 = trilinear.
 * dtype: 0 = float32, 1 = int32 (labels).                                       */
int msk_resample3d(msk_ctx* ctx, const void* src, int sd, int sh, int sw, void* dst,
                   int dd, int dh, int dw, int order, int dtype);
/* ---- loader augmentations on the device (medicalseg/transforms) ------- */
/* functional.py:103-110 resized_crop_3d: crop box (i,j,k)+(cd,ch,cw) of a (sd,sh,sw) volume,
 * zoomed to (dd,dh,dw) with msk_resample3d's coordinate map (order 1 image / 0 label,
 * transform.py:334-339).                                                              */
int msk_crop_resample3d(msk_ctx* ctx, const void* src, int sd, int sh, int sw, int i, int j,
                        int k, int cd, int ch, int cw, void* dst, int dd, int dh, int dw,
                        int order, int dtype);
/* functional.py:25-58 resize_3d / geometry.py:31-69 resample with order 3 == scipy.ndimage.zoom(order=3, mode='nearest',
 * grid_mode=False) of the crop box (ci,cj,ck)+(sd,sh,sw) of a DEVICE float32 volume [fd,fh,fw], to dst [dd,dh,dw] float32,
 * as tests/spline_reference.py states it, bit for bit: the box padded by 12 edge voxels per side (clamped to the BOX: the
 * reference crops first), the recursive B-spline prefilter in float64 along D, H, W (mirror initialisation, its sum cut
 * after 47 terms), then 4 x 4 x 4 taps around o * (n_in - 1) / (n_out - 1) + 12.  Every multiply and add is rounded on its
 * own.  work (DEVICE, 8-byte aligned): at least msk_spline_workspace(sd, sh, sw) bytes, (sd+24)(sh+24)(sw+24) doubles;
 * what it holds before the call does not matter and what it holds afterwards means nothing to the caller.  The query
 * needs no context and no GPU.  Four launches on the context stream (three prefilter passes, the zoom), nothing is
 * synchronised or downloaded.  Argument errors, reported before any launch: a null pointer, an extent < 1, a crop box
 * outside the volume, 2^31 voxels or more (volume, padded box or destination), a workspace that is misaligned, too small
 * or overlapping src / dst.  msk_resample3d / msk_crop_resample3d keep refusing order 3: integer volumes have none.      */
int msk_spline_workspace(int sd, int sh, int sw, size_t* bytes);
int msk_spline_resample3d(msk_ctx* ctx, const float* src, int fd, int fh, int fw, int ci, int cj, int ck, int sd, int sh,
                          int sw, float* dst, int dd, int dh, int dw, void* work, size_t work_bytes);
/* functional.py:80-88 flip_3d (np.flip along axis 0|1|2); out of place               */
int msk_flip3d(msk_ctx* ctx, const void* src, void* dst, int d, int h, int w, int axis,
               int dtype);
/* functional.py:91-100 rotate_3d == scipy.ndimage.rotate(angle, axes=(axis_a, axis_b),
 * order, mode='constant', cval, reshape=False): affine map about the plane centre in
 * double, no interpolation beyond the edges, int32 rounds half away from zero.       */
int msk_rotate3d(msk_ctx* ctx, const void* src, void* dst, int d, int h, int w, int axis_a,
                 int axis_b, double angle_deg, int order, double cval, int dtype);
/* values.py:67-87 HUnorm */
int msk_hu_norm(msk_ctx* ctx, const float* src, float* dst, size_t count, float hu_min,
                float hu_max, float hu_nan);
/* values.py:54-64 normalize; use_bounds==0 -> min/max of the volume */
int msk_minmax_norm(msk_ctx* ctx, const float* src, float* dst, size_t count, int use_bounds,
                    float min_val, float max_val);
/* transforms/transform.py:67-69: im / im.max() when max > 0 */
int msk_max_norm(msk_ctx* ctx, const float* src, float* dst, size_t count);
/* values.py:37-51 label_remap (sequential key->value passes) */
int msk_label_remap(msk_ctx* ctx, int32_t* label, size_t count, const int32_t* keys,
                    const int32_t* vals, int npairs);
/* transforms/functional.py:117-131 connected_component + RelabelComponent and
 * transform.py:343-396 BinaryMaskToConnectComponent / TopkLargestConnectComponent: n independent
 * contiguous d*h*w masks (dtype 0 = float32, 1 = int32; foreground = value != 0) -> int32 labels
 * in dst (same shape, not aliasing src) of the 6-connected components, 1, 2, ... by decreasing
 * size, ties by the first voxel in raster order; size < minimum_volume -> 0 and the later ranks
 * close up; k > 0 also zeroes every rank above k (k <= 0 keeps all).  status[n] (device, required)
 * receives per volume bit 0 = three or more distinct values (the reference's binary assert),
 * bit 1 = an internal iteration bound was hit; counts[n] (device, may be NULL) the number of kept
 * components.  Asynchronous: the caller reads status after synchronising.  n*d*h*w < 2^30;
 * scratch about 2.1 int32 words per voxel.                                                  */
int msk_connected_components3d(msk_ctx* ctx, const void* src, int32_t* dst, int n, int d, int h,
                               int w, int dtype, int minimum_volume, int k, int32_t* status,
                               int32_t* counts);
/* Hole filling: scipy.ndimage.binary_fill_holes (nnU-Net's create_nonzero_mask) and MONAI's FillHoles on n independent
 * contiguous d*h*w volumes; tests/fillholes_reference.py is the statement.  A voxel is zero when its value == 0 (float32: -0.0 is
 * zero, a NaN is not: msk_nonzero_bbox's rule).  The zero voxels form 6-connected components; a component is a HOLE when none
 * of its voxels lies on a face of the volume (an axis of extent 1 or 2 admits none).
 *   MSK_FILL_MASK   dst = 1 where src != 0 or the voxel lies in a hole, else 0 (dtype 0 = float32 or 1 = int32);
 *   MSK_FILL_LABEL  (dtype 1 only) dst = src, except that a hole whose non-zero 6-neighbours all carry ONE value c -- and,
 *                   with nclasses > 0, c is one of classes -- becomes c; a hole between two or more values stays 0.
 * dst (int32) may be src itself for dtype 1 (the last pass is elementwise and runs behind the last neighbour read); any other
 * overlap is an error.  classes: a HOST array of at most 64 values, read before the call returns; nclasses == 0 = any value;
 * only MSK_FILL_LABEL takes any.  status[n] (device, required): bit 1 = an internal iteration bound was hit
 * (msk_connected_components3d's bit; bit 0 is never set: there is no binary check).  counts[n] (device, may be NULL): the
 * number of voxels changed per volume.  Five launches on the context stream: the status / count words, msk_connected_components3d's
 * tile-local and face-merge union-find on the zero voxels, a pass that sends every root to its voxels and gathers per root
 * {touches a face, smallest, largest enclosing value} (merged per tile in LDS, integer atomics gated by an agent-scope load),
 * the elementwise apply with one count atomic per workgroup and volume.  Integer atomics only: the result does not depend on
 * the schedule.  Asynchronous: the caller reads status after synchronising.  n*d*h*w < 2^30; scratch from the context
 * workspace: 2 int32 words per voxel for MSK_FILL_MASK (link, flag), 4 for MSK_FILL_LABEL (link, flag, smallest, largest).
 * Argument errors, reported before any launch: an unknown dtype or mode, float32 with MSK_FILL_LABEL, an extent < 1, 2^30
 * voxels or more, a null src / dst / status, nclasses outside [0, 64] or without classes or without MSK_FILL_LABEL, dst
 * overlapping src other than dst == src for int32.                                                                          */
#define MSK_FILL_MASK 0
#define MSK_FILL_LABEL 1
#define MSK_FILL_NONE 2 /* dst = (src != 0) for either dtype: the apply pass alone, nothing is searched or filled, counts = 0 */
int msk_fill_holes3d(msk_ctx* ctx, const void* src, int32_t* dst, int n, int d, int h, int w, int dtype, int mode,
                     const int32_t* classes, int nclasses, int32_t* status, int32_t* counts);
/* utils/metric.py:21-61 calculate_area, as the confusion counts every hard-label metric (mean_iou, dice, accuracy,
 * kappa: metric.py:110-210) is a sum of.  pred / label: n contiguous volumes of voxels_per_volume int32 values
 * (4-byte alignment is enough).  counts (device): n rows of K*K + 1 unsigned 64-bit words, K = num_classes + 1:
 * word r*K + c = voxels with label class r and predicted class c among the voxels whose label is not ignore_index,
 * where class num_classes is "other" (a value < 0 or >= num_classes); the last word = voxels whose label is
 * ignore_index.  So intersect_area[i] = word (i, i), pred_area[i] = column i, label_area[i] = row i (+ the last word
 * when i == ignore_index).  accumulate != 0 adds to counts, 0 overwrites.  num_classes in [1, 64].  Exact (integer
 * atomics only), asynchronous, nothing data-dependent can fail.                                                  */
int msk_confusion3d(msk_ctx* ctx, const int32_t* pred, const int32_t* label, int n, long voxels_per_volume,
                    int num_classes, int ignore_index, unsigned long long* counts, int accumulate);
/* core/val.py:121-131,174 + utils/metric.py:64-107 auc_roc (sklearn.metrics.roc_auc_score of the softmax scores of the
 * whole validation set, one-vs-rest): stage 1 of 2.  probs: the output of msk_softmax_c, V = n*d*h*w voxels of C = probs.c
 * scores; label: V int32 class indices.  keys (device): C streams of `capacity` 32-bit words, class-major; the call writes
 * keys[c * capacity + offset + v] = bits(probs[v][c]) | (label[v] == c) << 31 for every class, -0.0 folded onto +0.0
 * (offset + V <= capacity < 2^31).  status (device, two 64-bit words, zeroed by the caller once): [0] += voxels whose label
 * is outside [0, C), [1] += scores that are negative or not finite (their keys are meaningless).  Asynchronous, no host
 * synchronisation; the inputs are not modified.                                                                        */
int msk_auc_pack(msk_ctx* ctx, msk_tensor probs, const int32_t* label, uint32_t* keys, long capacity, long offset,
                 unsigned long long* status);
/* bytes of scratch msk_auc_counts needs for `count` keys per class (host arithmetic only: no context, no GPU): a second key
 * buffer of 4 * classes * count bytes plus the histograms of the sort, about 1/16 of that.  count in [1, 2^31), classes
 * in [1, 64].                                                                                                          */
int msk_auc_workspace(long count, int classes, size_t* bytes);
/* core/val.py:121-131,174 + utils/metric.py:64-107 auc_roc, stage 2 of 2: sorts the first `count` keys of every class in
 * place (radix sort on bits 0-30, bit 31 carried; the sorted buffer is still a valid bag of keys that msk_auc_pack may
 * append to) and writes out[c] = {U2, n_pos, n_neg} (device, classes x 3 unsigned 64-bit words) with
 *   U2 = sum over the positives i of 2 * #{negatives with a smaller score} + #{negatives with an equal score},
 * so that AUC(c) = U2 / (2 * n_pos * n_neg).  Exact integers, independent of the schedule; asynchronous.  workspace:
 * device memory of at least msk_auc_workspace(count, classes) bytes, 16-byte aligned.                                  */
int msk_auc_counts(msk_ctx* ctx, uint32_t* keys, long capacity, long count, int classes, void* workspace,
                   size_t workspace_bytes, unsigned long long* out);
/* Boundary metrics (Hausdorff, HD95, average symmetric surface distance; the reference has none: medpy's conventions,
 * utils/metric.py surface_distances), stage 1: exact squared Euclidean distance transform of the int32 volume vol[d][h][w]
 * (axes z, y, x).  Features = the voxels with vol == cls, or with surface_only != 0 their surface: the voxels of that set
 * with at least one of the six face neighbours outside it (beyond the volume's edge counts as outside).  spacing (HOST
 * pointer, nullable = 1, 1, 1): sz, sy, sx; w_ = spacing_^2 rounded once.  dist2 (device, d*h*w doubles) receives
 *   min over the features of fl(fl(fl(wx dx^2) + fl(wy dy^2)) + fl(wz dz^2)),   +inf when there is no feature,
 * every fl one float64 rounding and no fused multiply-add: exactly the bits of the brute-force minimum, which the three
 * separable passes (x, y, z; three launches, in place in dist2, no other scratch) reproduce because rounding is monotone.
 * Extents 1 .. MSK_EDT_MAX_EXTENT per axis, spacing > 0 with its square in [1e-300, 1e300]; anything else is an error.
 * Asynchronous; vol is not modified.                                                                                    */
#define MSK_EDT_MAX_EXTENT 2048
int msk_edt3d(msk_ctx* ctx, const int32_t* vol, int d, int h, int w, int cls, int surface_only, const double* spacing,
              double* dist2);
/* *count (device, one unsigned 64-bit word, overwritten) = number of surface voxels of {vol == cls} (definition above):
 * the capacity msk_surface_gather needs.  Asynchronous.                                                                */
int msk_surface_count(msk_ctx* ctx, const int32_t* vol, int d, int h, int w, int cls, unsigned long long* count);
/* stage 2: out[0 .. min(*count, capacity)) = dist2[v] at every surface voxel v of {vol == cls}, in no particular order
 * (the host sorts); *count (device, overwritten) = the number of surface voxels, also when it exceeds capacity -- nothing
 * is written beyond capacity.  With dist2 = msk_edt3d of the OTHER mask's surface these are the directed squared surface
 * distances.  Asynchronous; vol and dist2 are not modified.                                                             */
int msk_surface_gather(msk_ctx* ctx, const int32_t* vol, int d, int h, int w, int cls, const double* dist2, double* out,
                       long capacity, unsigned long long* count);

/* Bias gradient of a convolution that feeds a BatchNorm, from the sums msk_affine_act_bwd_reduce
 * already produced (no extra pass over dy): with batch statistics sum_v dy[v][c] is identically 0
 * (the BN backward removes the mean) -- callers skip db there; with running statistics (eval-mode
 * BN, vnet.py:351-397 alignment runs) it is scale[c] * sums[c].                          */
int msk_bn_bias_grad(msk_ctx* ctx, int C, const float* sums, const float* scale, float* dbias,
                     int accumulate);
/* Adjoint of the residual join out = prelu(a + b, alpha) (vnet.py:110-111,154) in ONE pass:
 * da = dout * prelu'(a+b); db (+)= the same; dalpha[c] += sum dout*(a+b) over a+b <= 0.
 * (A join has no BatchNorm, so its data gradient needs no reduction first.)  float4-aligned
 * tensors with C % 4 == 0.                                                              */
int msk_add_act_bwd(msk_ctx* ctx, msk_tensor a, msk_tensor b, const float* alpha, msk_tensor dout,
                    msk_tensor da, msk_tensor db, int db_accumulate, float* dalpha);
/* The residual join right behind a conv -> BatchNorm -> PReLU unit (vnet.py:107-111, 150-154: the last LUConv of a stage and
 * relu2(add(out, down))) in ONE pass over the convolution output y, without materialising the unit's activation:
 *   out = prelu(prelu(scale*y + shift, alpha_inner) + res, alpha_outer)            (saves 8 bytes per element of traffic)
 * and its backward: da = gradient w.r.t. the unit's (never stored) activation, dres (+)= the same, dalpha_outer += ...;
 * the unit's own backward (msk_affine_act_bwd_reduce / msk_conv3d_bwd_bnact with dout = da) follows unchanged.        */
int msk_affine_act_join_fwd(msk_ctx* ctx, msk_tensor y, const float* scale, const float* shift, const float* alpha_inner,
                            msk_tensor res, const float* alpha_outer, msk_tensor out);
int msk_add_act_join_bwd(msk_ctx* ctx, msk_tensor y, const float* scale, const float* shift, const float* alpha_inner,
                         msk_tensor res, const float* alpha_outer, msk_tensor dout, msk_tensor da, msk_tensor dres,
                         int dres_accumulate, float* dalpha_outer);
/* the same pass additionally leaves the UNIT's backward sums (what msk_affine_act_bwd_reduce_ex(y, ..., dout = da) would
 * compute: unit_sums[0..3C) = sum du, sum du*xhat, d alpha_inner; unit_sums needs 4*C floats) and maxes (nullable, as in
 * msk_affine_act_bwd_reduce_ex): the unit's reduce pass is not needed afterwards.                                      */
int msk_add_act_join_bwd_ex(msk_ctx* ctx, msk_tensor y, const float* scale, const float* shift, const float* alpha_inner,
                            msk_tensor res, const float* alpha_outer, const float* mean, const float* invstd, msk_tensor dout,
                            msk_tensor da, msk_tensor dres, int dres_accumulate, float* dalpha_outer, float* unit_sums,
                            float* maxes /*nullable*/);

/* ELUCons(elu=True) (vnet.py:25-29): paddle.nn.ELU(alpha) as its own pass (the shipped configs use PReLU, which is fused
 * into the BatchNorm kernels above).  out = x > 0 ? x : alpha*(exp(x)-1), in place allowed;
 * dx (+)= dout * (out > 0 ? 1 : out + alpha) -- the derivative from the OUTPUT. */
int msk_elu_fwd(msk_ctx* ctx, msk_tensor x, float alpha, msk_tensor out);
int msk_elu_bwd(msk_ctx* ctx, msk_tensor out, msk_tensor dout, float alpha, msk_tensor dx, int accumulate);

/* ---- deep supervision (models/vnet_deepsup.py:266-277) -------------- */
/* F.interpolate(d, size=x.shape[2:], mode='trilinear') of a conv3^3 head: align_corners=
 * False, align_mode=0 [PADDLE]: per axis ratio = in/out, src = max(ratio*(o+0.5)-0.5, 0),
 * i0 = floor(src), i1 = min(i0+1, in-1).  src/dst: NDHWC with equal n and c.         */
int msk_interp_trilinear_fwd(msk_ctx* ctx, msk_tensor src, msk_tensor dst);
/* Adjoint: ddst (gradient at the resized size) -> dsrc (head resolution); separable
 * gather passes, deterministic.  scratch: device buffer of >= msk_interp_scratch_bytes
 * (may be NULL when only the depth axis is resized).                                  */
int msk_interp_scratch_bytes(msk_ctx* ctx, msk_tensor src, msk_tensor dst, size_t* bytes);
int msk_interp_trilinear_bwd(msk_ctx* ctx, msk_tensor ddst, msk_tensor dsrc, int accumulate,
                             void* scratch, size_t scratch_bytes);
/* nnU-Net deep supervision scores every head at the head's own extent: the label [n, d, h, w] (device, int32) down-sampled by
 * nearest neighbour to `levels` (1 .. 8) extents in ONE launch.  extents (host): levels x {od, oh, ow}, each in 1 .. the
 * label's extent of that axis; dst (host): levels device pointers, level l of n*od*oh*ow int32.
 *   dst_l[n, z, y, x] = label[n, iz, iy, ix],  per axis i = ((2 o + 1) * in) / (2 * out)   (integer division)
 * which is the voxel-centre, extent-ratio geometry (align_corners=False) of msk_interp_trilinear_fwd, so it also serves an axis
 * without an integer stride (12 -> 9); out == in is a copy.  The values travel as 32-bit patterns: ignore_index and anything
 * else are neither interpreted nor clamped.  Errors (nothing is launched): an empty label, n*d*h*w >= 2^31, an axis longer than 32768 (the
 * index arithmetic is 32-bit), levels outside 1 .. 8, an extent outside 1 .. in, a null or misaligned pointer, a destination
 * that overlaps the label.  Nothing is downloaded and nothing synchronises (tests/pyramid_reference.py states the formula). */
int msk_label_pyramid(msk_ctx* ctx, const int32_t* label, int n, int d, int h, int w, int levels, const int32_t* extents,
                      int32_t* const* dst);

/* ---- data parallel (RCCL over xGMI; core/train.py:81-85 fleet DataParallel) ---- */
#define MSK_UNIQUE_ID_BYTES 128
int msk_dp_unique_id(char* id128);                       /* rank 0 */
int msk_dp_rccl_version(int* version);                   /* ncclGetVersion: e.g. 22703 for 2.27.3; no context, no GPU needed */
int msk_dp_init(msk_ctx* ctx, const char* id128, int rank, int world);
int msk_dp_allreduce_sum(msk_ctx* ctx, float* buf, size_t count);   /* joins the weight-gradient side stream first */
/* SyncBatchNorm backward sums (2*C floats, produced on the main stream): same reduction WITHOUT the join,
 * so the 24 per-step statistics exchanges do not serialise the side stream */
int msk_dp_allreduce_stats(msk_ctx* ctx, float* buf, size_t count);
/* Gradient buckets (the Paddle reducer's role behind core/train.py:82-85).  Where the sum runs depends on the arrangement
 * chosen with msk_set_option(ctx, "dp_mode", m) / env MSEGK_DP_MODE before msk_dp_init (measurements: msk_dp.hip):
 *   0 (default) on the compute stream, like msk_dp_allreduce_sum -- callers then send the whole buffer once after backward;
 *   2           on the context's COMMUNICATION stream with its own communicator (ncclCommSplit of the first): it starts after
 *               everything enqueued so far on the compute and weight-gradient streams, blocks neither, and never queues
 *               behind the SyncBatchNorm exchanges of the compute stream;
 *   1 / 3       on the communication stream with the one communicator (1: the statistics exchanges run there too).
 * msk_dp_wait makes the compute stream wait for all outstanding buckets (call it before the optimizer); msk_sync implies it. */
int msk_dp_allreduce_async(msk_ctx* ctx, float* buf, size_t count);
int msk_dp_wait(msk_ctx* ctx);
int msk_dp_allgather(msk_ctx* ctx, const float* send, float* recv, size_t count_per_rank);
int msk_dp_broadcast(msk_ctx* ctx, float* buf, size_t count, int root);
int msk_dp_barrier(msk_ctx* ctx);
int msk_dp_destroy(msk_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* MSEGK_H */
