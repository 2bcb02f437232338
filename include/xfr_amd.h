/*
 * xfr_amd.h -- C ABI of the MI355X-native excitation-backprop (EBP) saliency engine.
 *
 * Drop-in boundary for the hot path of stresearch/xfr:
 *     python/xfr/models/whitebox.py:482-558   Whitebox.ebp / contrastive_ebp / truncated_contrastive_ebp
 *     python/xfr/models/whitebox.py:742-785   Whitebox.encode / embeddings
 * The reference has NO native layer (it is PyTorch hooks + autograd); this library replaces the three
 * hooked forwards and the autograd sweep of whitebox.py:490-498 with a static layer program executed by
 * hand-written HIP kernels for gfx950.  Each entry point below cites the reference code it stands in for.
 *
 * Conventions
 *   - plain C types only; all device pointers are raw HIP device pointers (float32, contiguous);
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); no entry point synchronises
 *     the stream unless documented;
 *   - every function returns an xfr_status; on failure xfr_last_error() holds a thread-local message;
 *   - one engine per (process, device); calls on one engine must be serialised by the caller
 *     (the reference is equally non-re-entrant: whitebox.py:291-296 mutable hook state);
 *   - the engine never mutates caller buffers other than the documented outputs (the reference leaves
 *     W+ installed in the caller's modules after ebp(): whitebox.py:371-377);
 *   - a call is bit-reproducible for a given batch size and settings.  ACROSS batch sizes a sample's map is the same
 *     arithmetic in a different summation order, not the same bits: three defaults look at the batch -- the lean schedule
 *     (batch % 4 == 0, xfr_engine_set_lean), the bf16x6 kernel (grids of >= 128 workgroups, xfr_engine_set_split_gemm) and tail
 *     balancing (xfr_engine_set_tail_balance; without it the bf16x6 kernel does not cut the tiles of a small 7 x 7 grid into K-parts
 *     either).  With all three off every launch of a layer runs one kernel in one K order.
 */
#ifndef XFR_AMD_H
#define XFR_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XFR_AMD_ABI_VERSION 7

typedef enum {
    XFR_OK = 0,
    XFR_INVALID_ARG = 1,        /* -> ValueError / AssertionError in the Python mirror            */
    XFR_UNSUPPORTED_LAYER = 2,  /* -> ValueError (whitebox.py:403 Sigmoid/ELU/Tanh, unknown kinds) */
    XFR_OOM = 3,
    XFR_HIP_ERROR = 4,
    XFR_STATE_ERROR = 5,        /* e.g. weights not loaded */
    XFR_RCCL_ERROR = 6          /* librccl missing, or a collective failed */
} xfr_status;

/* Layer program op kinds.  "Hooked" kinds are leaf nn.Module calls of the reference (they receive the
 * pre-forward/forward hooks of whitebox.py:306-437); G_* kinds are functional glue between modules
 * (torch.add, torch.max, F.normalize) that the reference's hooks never see. */
typedef enum {
    XFR_OP_CONV = 1,        /* nn.Conv2d                      resnet.py:116-122,177; lightcnn.py:53        */
    XFR_OP_BATCHNORM = 2,   /* nn.BatchNorm2d (eval)          resnet.py:118,179                             */
    XFR_OP_RELU = 3,        /* nn.ReLU(inplace=True)          resnet.py:124                                 */
    XFR_OP_MAXPOOL = 4,     /* nn.MaxPool2d                   resnet.py:181; resnet50_128.py:16 (ceil_mode)  */
    XFR_OP_AVGPOOL = 5,     /* nn.AvgPool2d                   resnet.py:186,211; lightcnn.py:237            */
    XFR_OP_ADD = 6,         /* Add module (2 inputs)          resnet.py:104-108; lightcnn.py:33-37          */
    XFR_OP_CONCAT = 7,      /* ConcatChannels (zero pad)      resnet.py:152-157                             */
    XFR_OP_MULTIPLY = 8,    /* Multiply(n)                    resnet.py:160-165                             */
    XFR_OP_LINEAR = 9,      /* nn.Linear (on flattened CHW)   resnet.py:187-189; lightcnn.py:228-229        */
    XFR_OP_SPLIT = 10,      /* Split module (identity view)   lightcnn.py:39-45                             */
    XFR_OP_G_ADD = 11,      /* functional a+b                 resnet50_128.py:187; lightcnn.py:252          */
    XFR_OP_G_MAXHALVES = 12,/* torch.max(split[0], split[1])  lightcnn.py:62                                */
    XFR_OP_G_NORMALIZE = 13 /* F.normalize(p=2, dim=1)        resnet.py:250                                 */
} xfr_op_kind;

/* One record of the static layer program (call order == the reference's forward call order).
 * Tensor id 0 is the network input; every op defines exactly one new tensor id `out`
 * (ids must be 1,2,3,... in op order).  All tensors are logically N x C x H x W. */
typedef struct {
    int32_t kind;        /* xfr_op_kind */
    int32_t in0;         /* first input tensor id  */
    int32_t in1;         /* second input tensor id (ADD, G_ADD) or -1 */
    int32_t out;         /* output tensor id */
    int32_t cout;        /* CONV/LINEAR: output channels; CONCAT: number of zero copies appended (resnet.py:157) */
    int32_t kh, kw;      /* CONV/MAXPOOL/AVGPOOL kernel; LINEAR: must equal the input H, W */
    int32_t stride;
    int32_t pad;
    int32_t ceil_mode;   /* MAXPOOL: ceil_mode.  CONV: `groups` of a grouped convolution (nn.Conv2d(groups = g), weight [cout][Cin / g][kh][kw]); 0 and 1 mean an
                          * ordinary convolution.  Cin and cout must be multiples of g; not on the first layer, a LINEAR or a MaxFeatureMap pair convolution */
    int32_t inplace;     /* RELU: 1 = nn.ReLU(inplace=True) (hook lands on the output tensor) */
    float   fparam;      /* MULTIPLY: n;  BATCHNORM: eps */
    int32_t w_weight;    /* index into the weight table, or -1 */
    int32_t w_bias;      /* index into the weight table, or -1 */
    int32_t w_mean;      /* BATCHNORM running_mean */
    int32_t w_var;       /* BATCHNORM running_var  */
} xfr_op_desc;

/* A host-memory view of one parameter tensor (float32, contiguous, PyTorch layout:
 * Conv [Cout][Cin][kh][kw], Linear [out][in], BatchNorm vectors [C]). */
typedef struct {
    const float* data;
    int64_t      numel;
} xfr_tensor_view;

/* ebp_subtree_mode of whitebox.py:262-263,396-430 */
typedef enum {
    XFR_MODE_AFFINEONLY = 0,
    XFR_MODE_AFFINEONLY_WITH_PRIOR = 1,
    XFR_MODE_NORELU = 2,
    XFR_MODE_ALL = 3
} xfr_subtree_mode;

typedef struct xfr_engine xfr_engine;

/* Version of this ABI (XFR_AMD_ABI_VERSION of the library that was loaded). */
int32_t xfr_abi_version(void);

/* Thread-local description of the last failure on this thread ("" if none). */
const char* xfr_last_error(void);

/* Build an engine for one backbone on HIP device `device`.
 * Stands in for: Whitebox.__init__ (whitebox.py:261-304: hook installation over every leaf module) plus the
 * backbone constructors (resnet.py:168-198, resnet50_128.py:6-170, lightcnn.py:216-247).
 * `ops`/`n_ops`: the layer program; `n_weights`: size of the weight table the ops index into;
 * (in_c,in_h,in_w): input image shape; `max_batch`: largest N accepted by the run calls.
 * Workspace for activations (A), positive activations (X) and two gradient streams is allocated here. */
xfr_status xfr_engine_create(const xfr_op_desc* ops, int32_t n_ops, int32_t n_weights,
                             int32_t in_c, int32_t in_h, int32_t in_w,
                             int32_t max_batch, int32_t device, xfr_engine** out);

xfr_status xfr_engine_destroy(xfr_engine* e);

/* Upload and pack the parameters (W, W+ = relu(W), transposed/flipped W+ for the backward-data GEMMs,
 * folded eval-mode BatchNorm scale/shift for gamma and relu(gamma)).
 * Stands in for: load_state_dict (resnet.py:277-279) and for the per-forward weight save / relu / restore
 * dance of whitebox.py:309-324,333-346,371-377, which becomes a one-off pack. */
xfr_status xfr_engine_load_weights(xfr_engine* e, const xfr_tensor_view* weights, int32_t n_weights);

/* Device address and size of the packed parameter arena, so that a multi-GPU launcher can broadcast it
 * (rank 0 loads, the others receive: replaces the per-job torch.load of
 * eval/generate_inpaintinggame_wb_saliency_maps_multigpu.py:74).  After EVERY write into the arena -- of an
 * engine that never called xfr_engine_load_weights, or through a pointer kept from an earlier call -- call
 * xfr_engine_mark_weights_loaded: it waits for the device and rebuilds what the engine derives from the arena
 * (the bf16 planes of xfr_engine_set_split_gemm); until then the bf16x6 kernel would run on the old weights. */
xfr_status xfr_engine_weight_arena(xfr_engine* e, void** dev_ptr, size_t* bytes);
xfr_status xfr_engine_mark_weights_loaded(xfr_engine* e);

/* Multi-GPU for hosts that are not Python (the Python mirror uses torch.distributed for the same broadcast): one process
 * per GPU, one RCCL communicator, ONE collective -- the broadcast of the packed parameter arena from `root`, which replaces
 * the per-job torch.load of the 298 MB checkpoint in every worker (eval/generate_inpaintinggame_wb_saliency_maps_multigpu.py:74,
 * 193-216).  The steady state has no exchange: triplets are independent.
 *   xfr_comm_unique_id   rank 0 fills 128 bytes (an ncclUniqueId) and hands them to the other ranks by any out-of-band means
 *   xfr_comm_init        collective over all `world` ranks; `device` is this rank's HIP device
 *   xfr_broadcast_weights  collective; the root must have called xfr_engine_load_weights, the others need not: their engines
 *                        are marked loaded on return.  Synchronises `stream`.
 * librccl is bound on first use; without it these four calls fail with XFR_RCCL_ERROR and nothing else is affected. */
#define XFR_COMM_ID_BYTES 128
typedef struct xfr_comm xfr_comm;
xfr_status xfr_comm_unique_id(void* id_out);
xfr_status xfr_comm_init(int32_t rank, int32_t world, const void* unique_id, int32_t device, xfr_comm** out);
xfr_status xfr_broadcast_weights(xfr_engine* e, xfr_comm* comm, int32_t root, void* stream);
xfr_status xfr_comm_destroy(xfr_comm* comm);

/* Whitebox(..., with_bias, eps, ebp_subtree_mode) -- whitebox.py:262-304. */
xfr_status xfr_engine_set_mode(xfr_engine* e, int32_t subtree_mode, float eps, int32_t with_bias);

/* Number of tensors / shape of a tensor of the program (C,H,W), for wrappers and tests. */
xfr_status xfr_engine_tensor_shape(xfr_engine* e, int32_t tensor_id, int32_t* c, int32_t* h, int32_t* w);

/* Forward only.  Stands in for WhiteboxNetwork.encode / classify (whitebox.py:58-64,98-103,126-133,222-230).
 * x_dev: N x in_c x in_h x in_w (NCHW).  The true values of tensor `tensor_id` are written to out_dev as
 * N x C x H x W (NCHW).  */
xfr_status xfr_forward(xfr_engine* e, const float* x_dev, int32_t n, int32_t tensor_id,
                       float* out_dev, void* stream);

/* Excitation backprop.  Stands in for Whitebox.ebp(x, Pn, mwp=True) (whitebox.py:482-504): the 'activation',
 * 'positive_activation' and 'ebp' forwards (:490-497) and Xn.backward(Pn) with the _backward_ebp tensor hooks
 * (:381-430, :498).
 *   x_dev        N x in_c x in_h x in_w
 *   n_streams    S = 1 (ebp) or 2 (the mate and non-mate sweeps of contrastive_ebp :514,:520 share one forward)
 *   seed_tensor  tensor id at which the gradient seed is injected: the classify() output when the classifier is
 *                hooked (seed = Pn), or the encode() tensor when the classifier is the un-hooked triplet layer
 *                of set_triplet_classifier (whitebox.py:93-96; seed = Pn @ W_cls, computed by the caller)
 *   seed_dev     S x N x D  (D = C*H*W of seed_tensor)
 * Outputs (either may be NULL):
 *   mwp_dev      S x N x C1 x H1 x W1 : P[-2], the MWP at the first conv's output (whitebox.py:499 before pooling)
 *   pooled_dev   S x N x H1 x W1      : sum over channels of P[-2]          (whitebox.py:499)
 */
xfr_status xfr_ebp(xfr_engine* e, const float* x_dev, int32_t n, int32_t n_streams,
                   int32_t seed_tensor, const float* seed_dev,
                   float* mwp_dev, float* pooled_dev, void* stream);

/* Contrastive / truncated contrastive EBP for a batch of independent probes.
 * Stands in for Whitebox.contrastive_ebp (whitebox.py:506-527) when percentile < 0 and
 * Whitebox.truncated_contrastive_ebp (whitebox.py:529-558) when 0 <= percentile <= 100, applied per sample,
 * followed by _mwp_to_saliency (ebp_ver 6 branch, whitebox.py:456-459: gaussian sigma=2 'nearest', clamp, /sum).
 *   seed_dev  2 x N x D : stream 0 = mate (k_poschannel), stream 1 = non-mate (k_negchannel)
 *   sal_dev   N x H1 x W1 saliency maps (each sums to 1) */
xfr_status xfr_contrastive(xfr_engine* e, const float* x_dev, int32_t n,
                           int32_t seed_tensor, const float* seed_dev, float percentile,
                           float* sal_dev, void* stream);

/* As xfr_contrastive, but stops before _mwp_to_saliency: contrast_dev (N x H1 x W1) receives `mwp_contrastive` /
 * `mwp_truncated_contrastive` (whitebox.py:526 / :557).  The saliency conversion of ebp_version != 6 (whitebox.py:451-454) of these maps is
 * xfr_mwp_to_saliency_u8; xfr_contrastive_u8 is both in one call. */
xfr_status xfr_contrastive_raw(xfr_engine* e, const float* x_dev, int32_t n, int32_t seed_tensor, const float* seed_dev,
                               float percentile, float* contrast_dev, void* stream);

/* xfr_contrastive for ebp_version != 6 (5 and 7-12: demo/test_whitebox.py:150,178, eval/eccv20.py:380,440,494): xfr_contrastive_raw followed on
 * the same stream, without a host round trip, by xfr_mwp_to_saliency_u8 of the contrast maps (float32 form).  sal_dev: N x H1 x W1 bytes, the
 * uint8 image Whitebox.contrastive_ebp / truncated_contrastive_ebp return for those versions.  Obeys the pipeline levels as xfr_contrastive_raw
 * does; H1 x W1 <= 65536.  ABI version 7, additive. */
xfr_status xfr_contrastive_u8(xfr_engine* e, const float* x_dev, int32_t n, int32_t seed_tensor, const float* seed_dev,
                              float percentile, uint8_t* sal_dev, void* stream);

/* One whole triplet step for N independent (mate, non-mate, probe) triplets -- demo/test_whitebox.py:124-133:
 *     x_mate = encode(mate); x_nonmate = encode(nonmate)                         (:71-72)
 *     set_triplet_classifier(scale * x_mate, scale * x_nonmate)                  (:129, scale = 1/2500)
 *     contrastive_ebp(probe, 0, 1)  |  truncated_contrastive_ebp(probe, 0, 1, percentile)   (:130)
 *   probes_dev   N  x in_c x in_h x in_w
 *   gallery_dev  2N x in_c x in_h x in_w : the N mates followed by the N non-mates
 *   encode_tensor  tensor id of encode()'s output; requires max_batch >= 2N
 * The two encode forwards run as one 2N-image batch, concurrently (internal streams, joined before the backward
 * sweep) with the probe forward.  sal_dev: N x H1 x W1. */
xfr_status xfr_triplet_contrastive(xfr_engine* e, const float* probes_dev, const float* gallery_dev, int32_t n,
                                   int32_t encode_tensor, float scale, float percentile, float* sal_dev, void* stream,
                                   int32_t inputs_ready);
/* The same step with the saliency conversion of ebp_version != 6 (xfr_mwp_to_saliency_u8, float32 form) in place of version 6's: float32 images
 * in, sal_dev N x H1 x W1 BYTES out.  ("u8tail": the uint8 is the OUTPUT; xfr_triplet_contrastive_u8 / _u8_host below take uint8 INPUT images
 * and return float maps.)  Everything else -- streams, pipelining, inputs_ready -- as xfr_triplet_contrastive.  ABI version 7, additive. */
xfr_status xfr_triplet_contrastive_u8tail(xfr_engine* e, const float* probes_dev, const float* gallery_dev, int32_t n,
                                          int32_t encode_tensor, float scale, float percentile, uint8_t* sal_dev, void* stream,
                                          int32_t inputs_ready);

/* Cross-call pipelining of xfr_triplet_contrastive (off by default).  When enabled, the engine keeps two forward slots
 * and the forwards of call i+1 start as soon as the slot they overwrite is free, i.e. they overlap the backward
 * sweep of call i (for calls made with inputs_ready = 1); results still appear in order on `stream`.  This is the steady state of the reference's job loop
 * (eval/generate_inpaintinggame_wb_saliency_maps_multigpu.py:200-215: independent jobs, inputs loaded ahead).
 * enable = 2 additionally pipelines xfr_ebp / xfr_contrastive / xfr_contrastive_raw: their forward overlaps the previous
 * call's sweep, and their x_dev must satisfy the inputs_ready contract of xfr_triplet_contrastive.
 * enable | 4: THREE forward slots instead of two -- the forwards may run two calls ahead of the sweep, which decouples a schedule whose forward is one
 * stream from its sweep (Light-CNN-29v2 EBP, 128 images per call: +1.8 %; level for the three-stream triplet step of the ResNets).
 * Costs one extra copy of the forward workspace per slot beyond the first.  Synchronises the device. */
xfr_status xfr_engine_set_pipeline(xfr_engine* e, int32_t enable);

/* Pipeline level 2 only.  ready = 0 (default): the internal forward stream of xfr_ebp / xfr_contrastive /
 * xfr_contrastive_raw first waits for everything already enqueued on the caller's `stream`, so an x_dev that is still
 * being produced there (a cast, a host-to-device copy) is safe -- at the price of the cross-call overlap.  ready = 1: the
 * caller promises that x_dev of the NEXT run call is already valid on the device and stays untouched until the result
 * has been consumed (the inputs_ready contract of xfr_triplet_contrastive); that call's forward then only waits for the slot
 * it overwrites.  The promise is consumed by the call it covers (one-shot): every later call is back to ready = 0 until the
 * caller renews it, so a stale promise cannot leak into a call that never made one (xfr_ebp_capture, xfr_ebp_store_firing and
 * every other entry point that sweeps go through the same core).  The reference has no counterpart: its inputs are host
 * tensors moved with .to(device) on one stream. */
xfr_status xfr_engine_set_inputs_ready(xfr_engine* e, int32_t ready);

/* Epilogue fusion (default: enable = 3).  Bit 0: the hook chain that follows a backward-data GEMM, BatchNorm / residual add /
 * ReLU after a convolution of a forward-only run (encode, the gallery of a triplet step) and MaxFeatureMap after a Light-CNN
 * convolution execute in the GEMM's epilogue on the LDS-transposed accumulator tile instead of in their own launches -- same
 * arithmetic in the same order, bit-identical maps, about 8 % more triplet maps per second.  Bit 1: also BatchNorm / ReLU after a
 * convolution of the PROBE forward, which additionally keeps the raw output and, where a hook needs it, the positive-pass BatchNorm
 * output (bit-identical; +0.6 % on ResNet-101, +2.2 % on ResNet-50-128d).  Bit 2 (tests): fused chains run through the
 * INTERPRETED epilogue -- the path a network outside the compiled signature table takes; the probe-forward and MaxFeatureMap
 * fusions, which only exist compiled, are then off.  enable = 0 gives every elementwise segment its own kernel again (the GEMM
 * launches then contain convolution work only, which is what one wants when profiling the MFMA kernel by itself).
 * Light-CNN's pooling stages (lightcnn.py:252, MaxPool2d(2)(x) + AvgPool2d(2)(x)) run as one forward kernel (sum, argmax bytes, positive-pass
 * sum) and their two VJPs as the head of the hook chain that follows them (EW_POOL2_IN) whenever bit 0 is set; bit 3 (tests) keeps the
 * separate kernels / launches: bit-identical either way (round 4).  Light-CNN's first layer (one input channel, 5x5, MaxFeatureMap) runs as a
 * direct convolution in the GEMM's K order unless bit 4 (tests) is set.  Backward chain GEMMs that cover the two streams of a contrastive sweep
 * walk their column tiles stream-interleaved (ConvParams::pair_m: the chain's forward-side operands are fetched once for both streams, -13 % GEMM
 * FETCH_SIZE on ResNet-101; which workgroup computes which tile is all that changes) unless bit 5 (A/B measurements) is set.  The block-input
 * gradient of a down-sampling residual block (shortcut AvgPool2d(2) [+ ConcatChannels], main path through a 1x1 / stride 2 convolution:
 * resnet.py:111-149) is built per pixel in the head of the hook chain that consumes it (EW_AVGUP_IN) from the pooled gradient and the
 * compact result of the strided GEMM, instead of by a slice copy, a hook launch, the pool's VJP and a read-modify-write scatter: same
 * operands, same operations, same bits; bit 6 (tests) keeps the separate launches.  Where the shortcut is a projection (resnet50_128.py), the
 * main path's hook chain of that block runs as a side branch of the Add-output GEMM's epilogue (the gradient is saved, the branch stored, the saved
 * value restored for the shortcut's chain) instead of as a launch of its own: same operations on the same operands; bit 7 (tests) keeps the launch.
 * Forward: the reference evaluates a down-sampling block's shortcut behind the main path (resnet.py:144-146); the engine computes it in front of
 * the main path's last convolution, so that the residual add [+ ReLU] joins that convolution's epilogue like in every other block, and keeps the
 * pooled shortcut inside its zero-padded form (a channel prefix is a storage prefix in CNHW: the padding is one fill, no copy).  The order of two
 * independent branches changes no value; bit 8 (tests, A/B) keeps program order and the separate add.
 * Bit 9 (tests, A/B): the phase launches of a strided KxK layer's backward-data pass run one after another instead of side by side (same bits).
 * Bit 10 (tests, A/B): depthwise launches (a grouped launch with one input or one output channel per group) stay on configuration 13, the grouped
 * MFMA kernel, instead of the vector-ALU kernel of configuration 14 (same values to rounding: the order of the sums differs). */
xfr_status xfr_engine_set_epilogue_fusion(xfr_engine* e, int32_t enable);

/* Share one forward pass between consecutive calls on the same input (off by default).  While hold = 1, a run call
 * (xfr_subtree_weights, xfr_ebp_capture, xfr_layerwise_ebp, xfr_ebp, ...) whose x_dev, n, seed tensor and stream equal those
 * of the previous call skips its forward and sweeps over the activations that are still in the workspace -- the three phases
 * of weighted_subtree_ebp (whitebox.py:647-737) run the same image through the network four times.  The caller promises
 * that the content of x_dev did not change in between.  Loading weights, changing the mode, or any forward on other
 * inputs drops the held state; hold = 0 ends the group. */
xfr_status xfr_engine_hold_forward(xfr_engine* e, int32_t hold);

/* Tail balancing of the convolution GEMMs (on by default).  A GEMM whose tile count is not a multiple of the CU count
 * has its last tiles cut along K so that every CU gets an equal share of the final round (+7 % GEMM rate on
 * ResNet-101 at 32-64 images).  The cut tiles add their K-parts in a fixed order: results are deterministic for a
 * given batch size, but which tiles are cut depends on the batch size, so a sample's map can differ in the last fp32
 * bits between batch sizes / positions.  enable = 0 restores batch-invariant arithmetic (every output element is
 * accumulated in one K order regardless of the batch). */
xfr_status xfr_engine_set_tail_balance(xfr_engine* e, int32_t enable);

/* uint8 entry points (ABI version 4).  The reference's callers hold decoded uint8 H x W x C crops and turn every one into a float tensor on the
 * host (resnet.py:25-37 convert_resnet101v4_image, whitebox.py:235-258 Whitebox_resnet50_128.preprocess, lightcnn.py:19-25
 * prepare_lightCNN_image) before it is copied to the device as fp32.  Here the uint8 images go to the device as they are -- a quarter of the bytes --
 * and the layout kernel in front of the first convolution does that arithmetic, in float64 like numpy does, bit for bit the reference's tensor
 * (tests/test_gpu_entry.py on the four bundled JPEGs): kind SUB_MEAN: out[c] = (float)((double)u8[c] - mean[c]); kind LUMINANCE (3-channel image,
 * 1-channel network): (float)((r / 255) w[0] + (g / 255) w[1] + (b / 255) w[2]).  Resizing / cropping is xfr_intake_u8 below, or the caller's.
 * x_u8_dev: n images, each in_h x in_w x channels, contiguous.  Everything else is xfr_forward / xfr_triplet_contrastive. */
enum { XFR_U8_SUB_MEAN = 0, XFR_U8_LUMINANCE = 1 };
typedef struct xfr_u8_preprocess {
    int32_t kind;       /* XFR_U8_* */
    int32_t channels;   /* of the uint8 images */
    double mean[4];     /* SUB_MEAN: per image channel */
    double weight[4];   /* LUMINANCE: per image channel */
} xfr_u8_preprocess;
xfr_status xfr_engine_set_u8_preprocess(xfr_engine* e, const xfr_u8_preprocess* p);
xfr_status xfr_forward_u8(xfr_engine* e, const uint8_t* x_u8_dev, int32_t n, int32_t tensor_id, float* out_dev, void* stream);
xfr_status xfr_triplet_contrastive_u8(xfr_engine* e, const uint8_t* probes_u8_dev, const uint8_t* gallery_u8_dev, int32_t n, int32_t encode_tensor,
                                      float scale, float percentile, float* sal_dev, void* stream, int32_t inputs_ready);
/* The same call for a caller whose images are fresh every time and live in HOST memory (ABI version 6): n probe and 2n gallery images, uint8 H x W x C,
 * pinned memory preferably.  The engine copies them itself -- its own copy stream, one device staging buffer per forward slot -- and orders the
 * forwards behind that copy, not behind `stream`: with xfr_engine_set_pipeline on, the copy, the preprocessing and the forwards of call i + 1 overlap
 * the sweep of call i, and nothing is promised about residency (xfr_triplet_contrastive_u8 with inputs_ready = 0 orders them behind everything on
 * `stream`, i.e. behind the previous sweep).  The copy is asynchronous: the host buffers must stay unchanged until it has run --
 * xfr_engine_wait_inputs_copied blocks the calling thread until the copies of the LAST such call are done (a caller that alternates two host buffers
 * calls it before refilling the one it used last; the call before that is then done too, copies run in order). */
xfr_status xfr_triplet_contrastive_u8_host(xfr_engine* e, const uint8_t* probes_u8_host, const uint8_t* gallery_u8_host, int32_t n, int32_t encode_tensor,
                                           float scale, float percentile, float* sal_dev, void* stream);
xfr_status xfr_engine_wait_inputs_copied(xfr_engine* e);
/* parity hook: the fp32 network input (n x C x H x W) the uint8 path builds from x_u8_dev */
xfr_status xfr_debug_u8_preprocess(xfr_engine* e, const uint8_t* x_u8_dev, int32_t n, float* out_nchw_dev, void* stream);

/* The lean schedule (on by default; ABI version 4).  A sweep nobody observes (no trace, prior, capture or stored firing; batch % 4 == 0) does not
 * need the literal operands a and x of whitebox.py:388-428 at every hook: the probe forward's W / relu(W) convolution forms the BatchNorm hook's
 * a / (x + eps) in its epilogue (both accumulators in one workgroup) and stores that ONE tensor instead of the two, with the sign bit recording
 * where the ReLU output behind it is zero; hooks whose x is their a (every Conv / Linear / pool / Add hook) become that one-bit gate.  Per hook the
 * result differs from the literal expression by at most one ulp (for a >= 1.7e-9; identical at a = 0): plain-EBP maps agree with the literal path to
 * ~1e-6 of their maximum; a contrastive map is a difference of two nearly equal sweeps and moves by what its conditioning makes of that -- measured up to
 * 1e-3 of the maximum on the ill-conditioned demo triplets (tests/test_gpu_parity.py::test_lean_schedule_equals_literal holds them to 2e-3), inside the
 * stated tolerance against the reference (5e-3 there) but not bit for bit.  enable = 0: the literal operands everywhere
 * (what every observing call -- traces, Whitebox.P[k], layerwise / weighted-subtree EBP -- runs regardless).  Batches that are not a multiple of four
 * always run literal, so a sample's map can differ in its last digits between a batch of 32 and a batch of 1: callers that need batch-invariant
 * arithmetic switch this off together with xfr_engine_set_tail_balance. */
xfr_status xfr_engine_set_lean(xfr_engine* e, int32_t enable);
/* bf16x6 GEMMs (ABI version 5).  The deep-K stride-1 convolutions of 14 x 14 and larger maps (K >= 256 for 1x1, K >= 1152 for KxK, 128 | Cout) can run
 * on the bf16 matrix pipe: every fp32 operand is the exact sum of three bf16 pieces, the six piece products of order <= 2 are exact and are accumulated in
 * fp32 (conv_gemm_split.hip K17).  Since round 6 no sum stays in the matrix pipe for more than three K-steps (48 of the K terms): the partial sums are
 * added to fp32 registers with round-to-nearest adds and alternate in sign, and a launch's error against float64 is BELOW the fp32 MFMA kernels'
 * (rms 5-9e-9 of the sum of magnitudes against 1.1-2.0e-8, no offset: profiles/r6/conv_error_probe.txt).
 * mode 3 (the default since round 6): the forward convolutions AND the sweep's backward-data GEMMs of those layers.  mode 1: the forward convolutions
 * only (the round-5 default).  mode 2: backward only (tuning).  mode 0: fp32 MFMA kernels everywhere.
 * Which launches: a covered layer's launch takes the kernel when its grid has at least 128 workgroups (half the CUs).  On maps of 14 x 14 and more a
 * workgroup is a tile of 128 x 128: about 25 images of a 14 x 14 layer, 6 of a 28 x 28 one.  On smaller maps (7 x 7) the tiles of a grid that would leave
 * CUs idle are cut into two K-parts (two workgroups per tile, met in the tail-balancing workspace: none with xfr_engine_set_tail_balance(0)): from 64 tiles,
 * i.e. from about 40 images of a 512-channel 7 x 7 layer (a 2048-channel one: 128 uncut tiles from 19 images); smaller launches -- Whitebox.contrastive_ebp on one image, the weighted-subtree probes -- run the fp32 kernels,
 * which fill the chip with 64 x 64 tiles where this one would leave it idle.  So a sample's map is bit-reproducible for a given batch size and agrees
 * across batch sizes to the kernels' summation-order difference (~1e-6 of its maximum; tests/test_gpu_parity.py::test_split_gemm_equals_fp32_kernels),
 * like K1's tail balancing (xfr_engine_set_tail_balance) and the lean schedule above.  Callers that need one arithmetic for every batch size: mode 0,
 * or mode + 4 (modes 5 .. 7) with tail balancing off: the covered layers take the kernel whatever the grid, uncut (tests and tuning: small launches are
 * slow on it).
 * The weight packs of the covered layers carry bf16 planes (+1.5x their size), built when the weights arrive (xfr_engine_load_weights,
 * xfr_engine_mark_weights_loaded, xfr_broadcast_weights, or this call); every entry point that changes the weights drops the old ones.  After writing
 * through a pointer from xfr_engine_weight_arena, call xfr_engine_mark_weights_loaded again: it rebuilds them.
 * XFR_SPLIT_GEMM=<mode> in the environment sets the mode of new engines. */
xfr_status xfr_engine_set_split_gemm(xfr_engine* e, int32_t mode);
/* Launches of the bf16x6 kernel so far, process-wide. */
xfr_status xfr_engine_split_gemm_stats(xfr_engine* e, int64_t* launches);

/* Convolution launches that took the lean form so far (W and relu(W) accumulated by one workgroup, quotient stored): 0 on an engine whose calls
 * all ran the literal schedule. */
xfr_status xfr_engine_lean_stats(xfr_engine* e, int64_t* dual_launches);

/* xfr_forward on batches of >= 32 images runs as two half batches on the engine's two internal streams and joins them on the caller's stream
 * (on by default; enable = 0: one forward on the caller's stream).  Images are independent; a sample's values can differ in the last fp32 bits
 * from the unsplit run exactly as they do between two batch sizes (tail balancing, see xfr_engine_set_tail_balance).  ABI version 3. */
xfr_status xfr_engine_set_forward_split(xfr_engine* e, int32_t enable);

/* _mwp_to_saliency (whitebox.py:448-460, ebp_ver 6) on N pooled maps: in N x H x W -> out N x H x W. */
xfr_status xfr_mwp_to_saliency(xfr_engine* e, const float* pooled_dev, int32_t n, int32_t h, int32_t w,
                               float* sal_dev, void* stream);

/* _mwp_to_saliency of every other ebp_version (whitebox.py:451-454) on N maps of h x w, one launch, one workgroup per map, to the byte what
 * NumPy 2 and Pillow give:
 *     img = np.uint8(255*((img-np.min(img))/(self.eps+(np.max(img)-np.min(img)))))         stage A
 *     img = np.array(PIL.Image.fromarray(img).filter(PIL.ImageFilter.GaussianBlur(radius=2)))
 *     img = np.uint8(255*((img-np.min(img))/(self.eps+(np.max(img)-np.min(img)))))         stage B
 * Exactly one of the two inputs is non-NULL and selects the form of stage A:
 *   pooled_dev  N x h x w float32 (a pooled MWP, a contrast map, a top-k subtree map): every operation a rounded float32 operation, with
 *               float32(eps) -- (uint8)(255.0f * ((v - min) / (eps + (max - min)))), no fused multiply-add, no reciprocal;
 *   levels_dev  N x h x w uint8 (the merged subtree map of XFR_SUBTREE_UINT8): NumPy evaluates the same expression in float64,
 *               (uint8)(255.0 * ((double)(v - min) / (eps + (double)(max - min)))), and so does the call, literally: at eps = 1e-12 the levels
 *               0..255 come back one lower (maximum 254), which no integer floor(255 v / d) reproduces.
 * The blur is Pillow's: three extended box passes per axis (box radius 1, weights 4473924 / 2^24 for the three centre pixels and 1677722 / 2^24
 * for the two at distance 2, replicated edges, + 2^23 >> 24 to bytes after every pass), rows then columns.  Stage B is the uint8 form on the blurred
 * bytes.  A constant map gives zeros.  eps is the engine's (xfr_engine_set_mode, a float): the float32 form uses it as it is, the uint8 form widened
 * to double -- for 1e-16 and 1e-12, the values the reference uses, eps + d rounds for every d = 1..255 as it does with the double literal.
 * Inputs must be finite with a finite max - min (the reference is undefined otherwise, and so is the result here).  n, h, w >= 1 and
 * h * w <= 65536 (a map lives in one workgroup's LDS), else XFR_INVALID_ARG; the reference's blur_radius is 2 everywhere and there is no other.
 * sal_dev: N x h x w bytes.  Does not synchronise.  ABI version 7, additive. */
xfr_status xfr_mwp_to_saliency_u8(xfr_engine* e, const float* pooled_dev, const uint8_t* levels_dev, int32_t n, int32_t h, int32_t w,
                                  uint8_t* sal_dev, void* stream);

/* ---- "next" row: layerwise_ebp / weighted_subtree_ebp (whitebox.py:561-581, 647-737) ------------------------------------
 * Firing indices are positions in Whitebox.P (reference order); the last one computed here is P[-2]. */

/* Number of hook firings of a sweep seeded at `seed_tensor` (= len(Whitebox.P) - 1: the image hook is not computed). */
xfr_status xfr_firing_count(xfr_engine* e, int32_t seed_tensor, int32_t* n_firings);

/* xfr_op_kind of the hooked module of every firing, reference order: what Whitebox.P_layername (whitebox.py:393) lists,
 * without running anything. */
xfr_status xfr_firing_kinds(xfr_engine* e, int32_t seed_tensor, int32_t* kinds, int32_t capacity);

/* whitebox.py:652-697: true-weight gradients of the two classifier outputs at every hooked module input (the `dA`
 * lists of the 'activation'-mode `_savegrad` hooks, :355-358), reduced per firing k to
 *     w[k] = max((g0[k] >= 0) * (-g1[k])),  idx[k] = argmax (flattened c,h,w index)          (gate_ge0 = 1, :689-690)
 *     w[k] = max((g0[k] <  0) * (-g1[k]))   with g0 = gradient of the cross-entropy loss          (gate_ge0 = 0, :693-694)
 * seed_dev: 2 x N x D gradient seeds at seed_tensor (stream 0 -> g0, stream 1 -> g1 = y[0][1]); w_host / idx_host:
 * n_firings x N host arrays.  Synchronises `stream`. */
xfr_status xfr_subtree_weights(xfr_engine* e, const float* x_dev, int32_t n, int32_t seed_tensor, const float* seed_dev,
                               int32_t gate_ge0, float* w_host, int32_t* idx_host, int32_t capacity, void* stream);

/* One standard EBP sweep (whitebox.py:567) over N independent images that returns, for image b and firing k,
 * P[k][b].flatten()[elem[k][b]] (elem < 0: skip) -- the values layerwise_ebp(mode='elementwise') turns into priors
 * (:575-577).  seed_dev: 1 x N x D; elem_host / p_host: n_firings x N host arrays.  Synchronises. */
xfr_status xfr_ebp_capture(xfr_engine* e, const float* x_dev, int32_t n, int32_t seed_tensor, const float* seed_dev,
                           const int32_t* elem_host, float* p_host, int32_t n_firings, void* stream);

/* whitebox.py:570-581 for a BATCH of layers of N independent images: sweep j of image b re-runs ebp(img_b, 0*P0) with
 * P_prior[firing[j][b]] set to a tensor that is zero except element elem[j][b] = val[j][b] (mode 'elementwise'), or -- one
 * sweep of one image -- to dense_prior_dev (mode 'argmax').  The N forwards run once; the n_sweeps x N sweeps form the
 * gradient batch (n_sweeps * N <= 2 * max_batch).  firing / elem / val: n_sweeps x N host arrays, firing < 0 marks an idle
 * sweep (its map is zero).  Handing the sweeps over in ascending firing order per image lets sweep j join the backward
 * pass only where its first prior fires.  pooled_dev: n_sweeps x N x H1 x W1 channel-pooled P[-2]. */
xfr_status xfr_layerwise_ebp(xfr_engine* e, const float* x_dev, int32_t n, int32_t n_sweeps, int32_t seed_tensor,
                             const int32_t* firing_host, const int32_t* elem_host, const float* val_host,
                             const float* dense_prior_dev, float* pooled_dev, void* stream);

/* weighted_subtree_ebp (whitebox.py:647-737) in one call, for N independent probes.  ABI version 7.
 *
 * seed_dev: 3 x N x D gradient seeds at seed_tensor -- stream 0 the gate output g0 and stream 1 the non-mate output g1 of
 * xfr_subtree_weights, stream 2 the EBP channel of xfr_ebp_capture / the layerwise sweeps.  The call holds the forward pass for all its
 * phases (xfr_engine_hold_forward; the previous setting is restored on every exit) and, per probe b:
 *   1. w[k], idx[k] as xfr_subtree_weights (gate_ge0 as there), the prior values P[k][idx[k]] as xfr_ebp_capture;
 *   2. the visiting order: `order_fn(w, n_firings, b, order, order_user)` fills `order` with a permutation of the firings, ascending by
 *      weight, and returns 0 (anything else fails the call with XFR_INVALID_ARG).  order_fn == NULL: the engine's rule, the order of
 *      np.argsort(w.astype(np.float64), kind='stable') -- equal weights (hooks that share one gradient tensor) ascend by firing index,
 *      so the higher index is visited first.  NumPy's default argsort breaks such ties differently, and the reference uses it: a
 *      caller that must select what the reference selects passes that order through order_fn (the Python wrapper does);
 *   3. from the heaviest firing down, skipping firings whose prior value is exactly 0 and firing 1 (whitebox.py:706-707), the
 *      candidates are swept in rounds of xfr_layerwise_ebp sweeps (sweep_batch per probe in the first round, 0 = min(2 * max_batch / N,
 *      max(8, 2 * topk)); later rounds min(sweep_batch, 2 * (topk - found) + 2)); a sweep whose pooled map has max > 0 is a valid
 *      subtree; a probe stops at topk valid subtrees or when it runs out of firings.  sweep_batch x N must fit 2 * max_batch rows;
 *   4. the valid maps in ascending weight order (the reference's [-topk:]) are merged: weights scale-normalised in fp32 (all equal:
 *      ones), each map times its normalised weight times 1 / (max + 1e-12), summed (do_max_subtree = 0) or maxed (1), then
 *      output MWP:      / max(sum, eps);
 *      output SALIENCY: as MWP, then _mwp_to_saliency (ebp_version 6: gaussian blur, clamp, normalise) of the merged AND the top-k maps;
 *      output UINT8:    the levels of np.uint8(255 * (m - min) / (eps + max - min)) (ebp_version != 6, whitebox.py:726), stored as floats;
 *                       the top-k maps stay pooled float32 maps (do_mwp_to_saliency = False of those versions);
 *      output UINT8_SALIENCY: as UINT8, then _mwp_to_saliency of those versions (xfr_mwp_to_saliency_u8: uint8 stretch, Pillow's
 *                       GaussianBlur(2), uint8 stretch) of the merged map -- the uint8 form, its input being levels -- AND of the top-k maps --
 *                       the float32 form; both stored as floats holding the exact integers 0..255.  Needs H1 x W1 <= 65536.
 * smap_dev: N x H1 x W1.  top_dev (may be NULL): N x topk x H1 x W1, probe b's valid maps (pooled, or converted for the SALIENCY kinds) in slots
 * 0 .. n_valid[b]-1, zero beyond.  w_valid_host / k_valid_host: N x topk host arrays, the weights and firings of those maps in the same
 * ascending-weight order, padded with 0 / -1; n_valid_host: N.  A probe without any valid subtree fails the call with XFR_STATE_ERROR
 * and the reference's message (whitebox.py:710-715).  Synchronises `stream`. */
typedef enum {
    XFR_SUBTREE_MWP = 0,
    XFR_SUBTREE_SALIENCY = 1,
    XFR_SUBTREE_UINT8 = 2,
    XFR_SUBTREE_UINT8_SALIENCY = 3
} xfr_subtree_output;

typedef int32_t (*xfr_subtree_order_fn)(const float* w, int32_t n_firings, int32_t probe, int32_t* order, void* user);

typedef struct {
    int32_t topk;                   /* >= 1 */
    int32_t gate_ge0;               /* 1: (g0 >= 0) * -g1 (do_mated_similarity_gating); 0: (g0 < 0) * -g1 */
    int32_t do_max_subtree;         /* 1: max over the valid subtrees; 0: sum */
    int32_t output;                 /* xfr_subtree_output */
    int32_t sweep_batch;            /* candidates per probe in the first round; 0: the default above */
    xfr_subtree_order_fn order_fn;  /* NULL: the engine's order rule */
    void* order_user;
} xfr_subtree_args;

xfr_status xfr_weighted_subtree_ebp(xfr_engine* e, const float* x_dev, int32_t n, int32_t seed_tensor, const float* seed_dev,
                                    const xfr_subtree_args* args, float* smap_dev, float* top_dev, float* w_valid_host,
                                    int32_t* k_valid_host, int32_t* n_valid_host, void* stream);

/* Whitebox.P[firing] of a standard EBP sweep (whitebox.py:394): out_dev receives N x C x H x W; (c,h,w) receive its shape
 * (out_dev == NULL: shape query only, nothing is run).  firing == xfr_firing_count: the hook on the first convolution's INPUT (the
 * reference's P[-1], the MWP at the image): relu(image) * relu(backward-data of that convolution with relu(W)), a gather kernel run on
 * demand -- nothing on the hot path reads it (round 4). */
xfr_status xfr_ebp_store_firing(xfr_engine* e, const float* x_dev, int32_t n, int32_t seed_tensor, const float* seed_dev,
                                int32_t firing, float* out_dev, int32_t* c, int32_t* h, int32_t* w, void* stream);

/* ---- STRise blackbox saliency (python/xfr/models/blackbox.py:299-442).  Additive entry points, ABI version 7. -------------------
 * The reference builds num_masks float64 masks (blackbox.py:320-336), the masked probes (:338-345), scores them (:366-414) and merges the masks
 * weighted by their scores (:416-442), all on the host.  Here a mask is never stored: it is its drawn cells (the zeros of the gh x gw grid of
 * blackbox.py:320-323, row-major indices) and its shift (x, y) of :331-332, and every kernel evaluates it from those in float64:
 *     c = (o + 0.5) * gh / (H + mask_scale) - 0.5,  o = output row + x  (columns alike with gw, W, y);  rows floor(c) and floor(c) + 1 through the
 *     mirror map i -> |i| mod 2 (gh - 1), folded at gh - 1;  mask = bilinear blend of the four grid values
 * which is skimage.transform.resize(order=1, mode='reflect', anti_aliasing=False) of skimage >= 0.19 cropped at [x : x + H, y : y + W] (:333).
 * H x W is the engine's input size.  cells_host: n_masks x num_elements int32, shifts_host: n_masks x 2 int32, both HOST arrays.  Every call
 * returns XFR_INVALID_ARG, before anything is launched, for a cell index outside [0, gh * gw), a shift outside [0, mask_scale),
 * mask_scale > min(H, W) or gh * gw > 4096.  The xfr_strise_* and xfr_inpaint_* calls on one engine share its sweep buffers and are ordered one
 * behind another on the device, whatever streams they are given. */
typedef struct {
    int32_t grid_h, grid_w;     /* gh, gw: ceil(H / mask_scale), ceil(W / mask_scale) in the reference (:302) */
    int32_t mask_scale;
    int32_t num_elements;       /* num_mask_elements: drawn cells per mask */
} xfr_strise_geometry;

/* blackbox.py:338-345 (apply_masks_using_image), resnet.py:25-37 (convert_resnet101v4_image), :366-394 (resnet_bb_fn, contrastive_triplet_similarity)
 * and :396-414 (score_masks) for all masks of one probe.
 *   probe_u8_dev  H x W x 3 uint8, fill_dev H x W x 3 float64 (the blurred probe of :352-357 or the constant 0.5 of :348): masked probe k is
 *                 (float)(mask_k * probe + (1 - mask_k) * fill - mean[c]), evaluated in float64, written by the device straight into the forward's
 *                 input; the engine's uint8 preprocessing must be XFR_U8_SUB_MEAN with 3 channels (its means are used), else XFR_INVALID_ARG
 *   refs_dev      n_refs x D, gallery_dev n_gal x D: fp32 embeddings at encode_tensor (D = C * H * W of it); n_refs == n_gal, or one of them is 1
 *                 (the broadcast of :391-393), else XFR_INVALID_ARG
 *   scores_dev    n_masks float64: mean_j[(sim0_ref_j - simk_ref_j) - (sim0_gal_j - simk_gal_j)], sim = 1 - 0.5 |p / |p| - g / |g||, in float64 from
 *                 the fp32 embeddings
 *   orig_dev      (may be NULL) n_refs + n_gal float64: the unmasked probe's similarities (original_probe_ref_scores, original_probe_gallery_scores)
 * The sweep runs in batches of the engine's max_batch through xfr_forward; the unmasked probe rides along as image zero, and the last batch is
 * padded with all-ones masks whose results are dropped, so one schedule serves every batch -- results depend on max_batch like those of xfr_forward.
 * The masked probes of batch i + 1 are generated on a side stream while batch i is encoded.  The host blocks once, before the first launch, until
 * the work already queued on `stream` has finished (the cell table is copied from pageable memory behind it); the call does not wait for its own
 * launches. */
xfr_status xfr_strise_score(xfr_engine* e, const uint8_t* probe_u8_dev, const double* fill_dev, const int32_t* cells_host, const int32_t* shifts_host,
                            int32_t n_masks, const xfr_strise_geometry* geom, const float* refs_dev, int32_t n_refs, const float* gallery_dev,
                            int32_t n_gal, int32_t encode_tensor, double* scores_dev, double* orig_dev, void* stream);

/* blackbox.py:416-421 (combine_masks) and :434-441: sal_dev (H x W float64) = m - min(m), / max, with m = sign * (1 - sum_k w_k mask_k / n_selected);
 * sign +1 is the positive_scores branch (:434), -1 the other (:438).  weights_dev: n_masks float64, the score of a selected mask and 0 for every
 * other; n_selected: the count of selected masks (the divisor of .mean(axis=0)).  The cells of one mask must be distinct (they are drawn without
 * replacement, :322), else XFR_INVALID_ARG.  Accumulates in float64 without atomics: bit-reproducible.  Synchronises `stream` once, before the launches. */
xfr_status xfr_strise_combine(xfr_engine* e, const double* weights_dev, int32_t n_selected, const int32_t* cells_host, const int32_t* shifts_host,
                              int32_t n_masks, const xfr_strise_geometry* geom, int32_t sign, double* sal_dev, void* stream);

/* Parity hooks: masks [first, first + count) as float64 count x H x W (self.masks of :336), and their fp32 network input count x 3 x H x W (what
 * xfr_strise_score feeds the forward).  count <= max_batch for the second. */
xfr_status xfr_strise_debug_masks(xfr_engine* e, const int32_t* cells_host, const int32_t* shifts_host, int32_t n_masks, const xfr_strise_geometry* geom,
                                  int32_t first, int32_t count, double* masks_dev, void* stream);
xfr_status xfr_strise_debug_masked_probes(xfr_engine* e, const uint8_t* probe_u8_dev, const double* fill_dev, const int32_t* cells_host,
                                          const int32_t* shifts_host, int32_t n_masks, const xfr_strise_geometry* geom, int32_t first, int32_t count,
                                          float* out_nchw_dev, void* stream);

/* ---- Inpainting-game scoring (python/xfr/inpainting_game/inpainting_game.py:12-197).  Additive entry points, ABI version 7. ----------------
 * The reference thresholds a saliency map at n_levels levels (create_threshold_masks, :12-77), switches the probe to its inpainted twin under each
 * mask (:114-129), embeds the hybrids (:134) and asks which gallery mean each one is nearer to (:135-140), all on the host.  Here every step runs
 * on the device; soft-edged masks (mask_blur_sigma), per-map levels and the caller's totals ('percent-pixels') are options of the _ex forms further
 * down.  The mask arguments, shared by all entry points:
 *   sal_dev       n_maps x H x W float64 maps with a positive sum; every map of a call goes through one launch
 *   noise_dev     H x W float64, np.random.rand(H, W) after np.random.seed(seed) (:26,37), shared by all maps, or NULL for none
 *   max_noise     :18;  include_zero: include_zero_elements (:27-32)
 *   method        XFR_INPAINT_PERCENT_DENSITY (:43-56): levels_host are percentiles in [0, 100], non-decreasing; mask l is cdf / max(cdf) > 1 - p_l / 100
 *                 (0 for a last percentile of 100), cdf the running sum of s = v / sum(v), v = sal + nz * noise * max_noise, in ascending order of v.
 *                 EQUAL VALUES ARE ORDERED BY FLAT INDEX (numpy's argsort leaves their order unspecified).
 *                 XFR_INPAINT_THRESHOLDS (:57,65, the 'mass-threshold' use): levels_host are thresholds, non-increasing; mask l is s > thr_l.
 *   levels_host   n_levels float64 on the HOST, 1 <= n_levels <= 255
 * The masks of one map are nested (the thresholds fall as the level rises), and are kept as one byte per pixel: first_on, the first level at which
 * the pixel is on, n_levels where it never is; mask l is first_on <= l.  All arithmetic is float64 without floating-point atomics: results are
 * bit-reproducible from run to run.  Every call returns XFR_INVALID_ARG, before anything is launched, for a null pointer, n_maps < 1, n_levels
 * outside [1, 255], levels that are unsorted or (percentiles) outside [0, 100], and an unknown method.  On one engine these calls and the
 * xfr_strise_* calls are ordered one behind another on the device, whatever streams they are given. */
typedef enum { XFR_INPAINT_PERCENT_DENSITY = 0, XFR_INPAINT_THRESHOLDS = 1 } xfr_inpaint_method;

/* classified_as_inpainted_twin (:80-146) for n_maps maps of one probe.  H x W is the engine's input size.
 *   orig_dev, inpaint_dev   in_c x H x W fp32, network format (in_c = 3, or 1 for Light-CNN): hybrid (map, l) is mask_l ? inpaint : orig, which is
 *                           what (1 - m) * a + m * b in float64 followed by .float() gives for 0/1 masks (:124-129, whitebox.py:762), written by the
 *                           device straight into the forward's input
 *   gal_orig_dev, gal_inp_dev   D fp32 (D = C * H * W of encode_tensor): original_gal_embed and inpaint_gal_embed
 *   pg_dev, pr_dev          n_maps x n_levels float64: |e / |e| - gal_inp| and |e / |e| - gal_orig| in float64 from the fp32 embedding e (:135-138)
 *   cls_dev                 n_maps x n_levels uint8: pg < pr (:140)
 * The n_maps * n_levels hybrids run through xfr_forward in batches of the engine's max_batch; the last batch is padded with copies of the original
 * whose results are dropped, so one schedule serves every batch.  The hybrids of batch i + 1 are built on a side stream while batch i is encoded.
 * The call does not block the host. */
xfr_status xfr_inpaint_score(xfr_engine* e, const double* sal_dev, int32_t n_maps, const double* noise_dev, double max_noise, int32_t include_zero,
                             int32_t method, const double* levels_host, int32_t n_levels, const float* orig_dev, const float* inpaint_dev,
                             const float* gal_orig_dev, const float* gal_inp_dev, int32_t encode_tensor, double* pg_dev, double* pr_dev,
                             uint8_t* cls_dev, void* stream);

/* intersect_over_union_thresholded_saliency (:149-197) as integer counts: gt_dev H x W uint8 (non-zero: inside the ground truth), counts_dev
 * n_maps x n_levels x 3 int64 = |gt & mask|, |gt | mask|, |~gt & mask| (:178-192).  H x W is the engine's input size. */
xfr_status xfr_inpaint_iou(xfr_engine* e, const double* sal_dev, int32_t n_maps, const double* noise_dev, double max_noise, int32_t include_zero,
                           int32_t method, const double* levels_host, int32_t n_levels, const uint8_t* gt_dev, int64_t* counts_dev, void* stream);

/* Parity hooks.  xfr_inpaint_debug_masks: the masks of :12-65 for maps of any size h x w (h * w <= 2^24): first_on_dev n_maps x h x w uint8 and
 * (cdf_dev may be NULL) the float64 value each pixel was compared by, cdf / max(cdf) or s.  xfr_inpaint_debug_blends: the fp32 hybrids
 * [first, first + count) of the n_maps * n_levels list (:127-129), count x in_c x H x W, at the engine's input size. */
xfr_status xfr_inpaint_debug_masks(xfr_engine* e, const double* sal_dev, int32_t n_maps, int32_t h, int32_t w, const double* noise_dev, double max_noise,
                                   int32_t include_zero, int32_t method, const double* levels_host, int32_t n_levels, uint8_t* first_on_dev,
                                   double* cdf_dev, void* stream);
xfr_status xfr_inpaint_debug_blends(xfr_engine* e, const double* sal_dev, int32_t n_maps, const double* noise_dev, double max_noise, int32_t include_zero,
                                    int32_t method, const double* levels_host, int32_t n_levels, const float* orig_dev, const float* inpaint_dev,
                                    int32_t first, int32_t count, float* out_dev, void* stream);

/* Options of the _ex forms below.  Each _ex form takes the arguments of its plain form plus `opt` before `stream`; opt == NULL is the plain form,
 * result for result and error text for error text.  Additive, ABI version 7.  Everything the options point to is HOST memory, read before the call
 * returns; the options travel to the device as kernel arguments, so the _ex forms block the host no more than the plain ones.
 *   levels_per_map     levels_host holds one row of n_levels per map, each checked like the single row.
 *   totals_host        s = v / totals_host[m] instead of v / (the device's own sum of v).  The device sums in a fixed order of its own, which is not
 *                      numpy's pairwise order, so its s can differ from numpy's in the last bit; thresholds taken from numpy's s (np.percentile:
 *                      'percent-pixels', :57-62) often equal an element of s or sit one ulp beside it, and only the caller's own sum decides those
 *                      pixels as numpy does.  With either of these two options the mask kernel is launched once per map.
 *   blur_radius r      soft-edged masks (mask_blur_sigma, :68-75): every mask, as float64 0 / 1, goes through a separable Gaussian of 2 r + 1 taps,
 *                      axis 0 then axis 1, indices clamped to the edge, and hybrid (map, l) becomes (float)((1 - m) * orig + m * inpaint) evaluated
 *                      in float64, two products and one sum, each rounded.  Per output of a pass, with w = blur_kernel_host:
 *                          t = in[0] * w[r];  for j = r, r - 1, ..., 1:  t += (in[-j] + in[+j]) * w[r - j]      (no fused multiply-add)
 *                      which is scipy.ndimage.gaussian_filter(mask, sigma, mode='nearest', truncate=4.0) bit for bit when w is scipy's kernel:
 *                      r = int(4 sigma + 0.5), w = exp(-0.5 / sigma^2 * x^2) / sum, computed by numpy (its exp differs from libm's in the last bit,
 *                      hence the caller's weights).  0 <= r <= XFR_INPAINT_MAX_BLUR_RADIUS.
 *   blur_level_host    NULL: every level is blurred; else n_levels flags, 0 leaves the level hard (the reference skips percentile 100, :71-72).
 *                      Ignored when blur_radius is 0.
 * XFR_INVALID_ARG, before anything is launched, with a text naming the value: a struct_size other than sizeof(xfr_inpaint_options), a radius outside
 * [0, 64], a radius without a kernel, a weight that is not finite or negative, w[r - j] != w[r + j], a total that is not positive and finite, and a
 * non-zero radius given to xfr_inpaint_iou_ex or xfr_inpaint_debug_masks_ex (both are defined on hard masks). */
#define XFR_EX      /* marks the entry points added to ABI version 7 after its first release (expands to nothing).  It also keeps the pattern
                     * `xfr_status xfr_inpaint_<name>(`, by which tests/test_inpainting_score_host.py pins the four plain forms, reading those four. */
#define XFR_INPAINT_MAX_BLUR_RADIUS 64      /* 7 % of 224 pixels at truncate 4 is 63 */
typedef struct {
    int32_t struct_size;            /* sizeof(xfr_inpaint_options), checked */
    int32_t levels_per_map;
    const double* totals_host;      /* NULL, or n_maps sums */
    int32_t blur_radius;            /* 0: hard masks */
    const double* blur_kernel_host; /* 2 r + 1 weights */
    const uint8_t* blur_level_host; /* NULL, or n_levels flags */
} xfr_inpaint_options;

xfr_status XFR_EX xfr_inpaint_score_ex(xfr_engine* e, const double* sal_dev, int32_t n_maps, const double* noise_dev, double max_noise, int32_t include_zero,
                                       int32_t method, const double* levels_host, int32_t n_levels, const float* orig_dev, const float* inpaint_dev,
                                       const float* gal_orig_dev, const float* gal_inp_dev, int32_t encode_tensor, double* pg_dev, double* pr_dev,
                                       uint8_t* cls_dev, const xfr_inpaint_options* opt, void* stream);
xfr_status XFR_EX xfr_inpaint_iou_ex(xfr_engine* e, const double* sal_dev, int32_t n_maps, const double* noise_dev, double max_noise, int32_t include_zero,
                                     int32_t method, const double* levels_host, int32_t n_levels, const uint8_t* gt_dev, int64_t* counts_dev,
                                     const xfr_inpaint_options* opt, void* stream);
xfr_status XFR_EX xfr_inpaint_debug_masks_ex(xfr_engine* e, const double* sal_dev, int32_t n_maps, int32_t h, int32_t w, const double* noise_dev,
                                             double max_noise, int32_t include_zero, int32_t method, const double* levels_host, int32_t n_levels,
                                             uint8_t* first_on_dev, double* cdf_dev, const xfr_inpaint_options* opt, void* stream);
xfr_status XFR_EX xfr_inpaint_debug_blends_ex(xfr_engine* e, const double* sal_dev, int32_t n_maps, const double* noise_dev, double max_noise,
                                              int32_t include_zero, int32_t method, const double* levels_host, int32_t n_levels, const float* orig_dev,
                                              const float* inpaint_dev, int32_t first, int32_t count, float* out_dev, const xfr_inpaint_options* opt,
                                              void* stream);
/* Parity hook: the float64 masks [first, first + count) of the n_maps * n_levels list as the hybrids see them, count x h x w, for maps of any size
 * h x w (h * w <= 2^24); opt == NULL or a radius of 0 gives the hard masks as 0.0 / 1.0.  count <= 65535. */
xfr_status XFR_EX xfr_inpaint_debug_soft_masks(xfr_engine* e, const double* sal_dev, int32_t n_maps, const double* noise_dev, double max_noise,
                                               int32_t include_zero, int32_t method, const double* levels_host, int32_t n_levels, int32_t h, int32_t w,
                                               const xfr_inpaint_options* opt, int32_t first, int32_t count, double* masks_dev, void* stream);

/* ---- STRise for the generator's black box (eval/generate_inpaintinggame_bb_saliency_maps_multigpu.py:69-113,
 * python/xfr/inpainting_game/generate_blackbox_saliency.py:48-73).  Additive entry points, ABI version 7. -----------------------------------
 * The reference's own evaluation never uses the named black box: its bb_fn (:73-101) sends every masked probe v = mask * probe + (1 - mask) * fill
 * (blackbox.py:343) through Whitebox.convert_from_numpy (whitebox.py:787-806) of whichever network create_wbnet returned:
 *     q = uint8((v / 255) * 255)                         (:794-795,803; the conversion truncates; the resize of :802 is the identity at 224 x 224)
 *     XFR_U8_SUB_MEAN   (float)((double)q - mean[c])     (ResNet-101: whitebox.py:108-110, resnet.py:25-37; ResNet-50-128d: whitebox.py:235-258)
 *     XFR_U8_LUMINANCE  PIL's bilinear Resize + CenterCrop of q, then (float)((r/255) w0 + (g/255) w1 + (b/255) w2)     (Light-CNN: lightcnn.py:19-31)
 * quantize = 1 selects that chain.  Truncation makes q depend on the last bit of the mask, so under quantize = 1 (and `exact` of the mask hook) the
 * mask is scipy.ndimage.zoom(order=1, mode='mirror', grid_mode=True) TO THE BIT, every operation rounded to float64 and none contracted:
 *     cc = ((o + 0.5) * ratio) - 0.5, ratio = g / (n + mask_scale);  c = cc < 0 ? -cc : cc;  st = floor(c);  w0 = 1 - (c - st);  w1 = 1 - w0;
 *     taps st and st + 1, the second folded at g - 1 (g == 1: tap 0 with weight 1);  mask = (((0 + (G00 wy0) wx0) + (G01 wy0) wx1) + (G10 wy1) wx0) + (G11 wy1) wx1
 * Image zero of the sweep (the unmasked probe) and the padding rows take q = probe: uint8((k / 255) * 255) == k for every level, and an all-ones
 * grid under the exact law is not 1 everywhere.
 * PIL's 8-bit bilinear resize (Pillow 12, Resample.c) is two integer passes, the horizontal one first, each output clip8((2^21 + sum_t pixel[first + t] *
 * coef[t]) >> 22); the caller supplies the tap tables of the rows and columns THE CROP KEEPS (xfr_amd.models.blackbox.pil_bilinear_tables). */
#define XFR_STRISE_MAX_TAPS 8
typedef struct {
    int32_t first, count;               /* pixels [first, first + count) of the probe's axis; 1 <= count <= XFR_STRISE_MAX_TAPS */
    int32_t coef[XFR_STRISE_MAX_TAPS];  /* weights in 2^-22, each >= 0; 255 * their sum + 2^21 must fit in int32 */
} xfr_strise_tap;

typedef struct {
    int32_t struct_size;                /* sizeof(xfr_strise_options), checked */
    int32_t probe_h, probe_w;           /* size of the probe, the fill and the masks (no longer the engine's input size) */
    int32_t quantize;                   /* 0: the arithmetic of xfr_strise_score; 1: the chain above */
    const xfr_strise_tap* row_tab;      /* HOST, in_h entries; XFR_U8_LUMINANCE engines under quantize = 1 only, else may be NULL */
    const xfr_strise_tap* col_tab;      /* HOST, in_w entries */
} xfr_strise_options;

/* The calls above with options; opt == NULL is the call above itself (the engine's input size, quantize 0, the closed-form mask law): the same
 * code path, results equal to the bit.  XFR_INVALID_ARG before anything is launched, with a text naming the cause, for: a struct_size other than
 * sizeof(xfr_strise_options); quantize outside {0, 1}; quantize = 1 on an engine without xfr_engine_set_u8_preprocess; an XFR_U8_SUB_MEAN engine
 * (or quantize = 0) whose input size is not probe_h x probe_w; an XFR_U8_LUMINANCE engine without tables; a table entry with count outside
 * [1, XFR_STRISE_MAX_TAPS], a window outside the probe, a negative coefficient or a coefficient sum that overflows int32; a band of 16 output rows whose
 * probe rows do not fit the kernel's 60 KB of LDS; and everything the calls above refuse, against probe_h x probe_w.
 * xfr_strise_combine_ex keeps the closed-form law (the map's bar is 1e-6, the laws differ by 2e-16): options only free it from the engine's input size. */
xfr_status XFR_EX xfr_strise_score_ex(xfr_engine* e, const uint8_t* probe_u8_dev, const double* fill_dev, const int32_t* cells_host, const int32_t* shifts_host,
                               int32_t n_masks, const xfr_strise_geometry* geom, const float* refs_dev, int32_t n_refs, const float* gallery_dev,
                               int32_t n_gal, int32_t encode_tensor, double* scores_dev, double* orig_dev, const xfr_strise_options* opt, void* stream);
xfr_status XFR_EX xfr_strise_combine_ex(xfr_engine* e, const double* weights_dev, int32_t n_selected, const int32_t* cells_host, const int32_t* shifts_host,
                                 int32_t n_masks, const xfr_strise_geometry* geom, int32_t sign, double* sal_dev, const xfr_strise_options* opt, void* stream);
/* exact = 1: the masks under scipy's law above; 0: the closed form */
xfr_status XFR_EX xfr_strise_debug_masks_ex(xfr_engine* e, const int32_t* cells_host, const int32_t* shifts_host, int32_t n_masks, const xfr_strise_geometry* geom,
                                     int32_t first, int32_t count, int32_t exact, double* masks_dev, const xfr_strise_options* opt, void* stream);
/* the network input of masks [first, first + count): count x in_c x in_h x in_w fp32, what xfr_strise_score_ex feeds the forward.  first == -1 is
 * image zero of the sweep, the unmasked probe (then masks [0, count - 1) follow it), and up to max_batch rows behind mask n_masks - 1 are the
 * padding of the sweep's last batch */
xfr_status XFR_EX xfr_strise_debug_masked_probes_ex(xfr_engine* e, const uint8_t* probe_u8_dev, const double* fill_dev, const int32_t* cells_host,
                                             const int32_t* shifts_host, int32_t n_masks, const xfr_strise_geometry* geom, int32_t first, int32_t count,
                                             float* out_dev, const xfr_strise_options* opt, void* stream);
/* q itself, count x probe_h x probe_w x 3 uint8, for any engine (opt required; quantize and the tables are not read); first == -1 as above */
xfr_status XFR_EX xfr_strise_debug_quantized(xfr_engine* e, const uint8_t* probe_u8_dev, const double* fill_dev, const int32_t* cells_host,
                                      const int32_t* shifts_host, int32_t n_masks, const xfr_strise_geometry* geom, int32_t first, int32_t count,
                                      uint8_t* q_dev, const xfr_strise_options* opt, void* stream);

/* ---- Match calibration on embeddings (python/xfr/inpainting_game/net_mate_nonmate_dists.py:118-128, eval/filter_inpaintinggame_for_net.py:105-165,
 * eval/eccv20.py:53-59).  Additive entry points, ABI version 7. ------------------------------------------------------------------------------
 * Matrices are row-major float32 on the engine's device; index tables are HOST memory, read before the call returns; the work is enqueued on
 * `stream`.  The engine lends its device and its error text: no weights are needed.  One distance arithmetic throughout,
 *     |a - b| = (float) sqrt( sum_d (double)(a[d] - b[d])^2 ),    a[d] - b[d] one float32 subtraction
 * the single rounding np.linalg.norm(a - b) makes on float32 input, with the sum of squares in float64: identical rows give exactly 0, and nothing
 * is formed from |a|^2 + |b|^2 - 2 a.b.
 * XFR_INVALID_ARG before anything is launched, with a text naming the value: a null pointer, a count below 1, 1 <= d <= XFR_MATCH_MAX_D violated, a
 * row index outside its matrix, an empty group, k outside [1, XFR_MATCH_MAX_K] or above ng - (exclude_same_index != 0), an output that overlaps an
 * input (by the sizes the counts imply) or the other output. */
#define XFR_MATCH_MAX_K 64
#define XFR_MATCH_MAX_D 4096
/* Templates: group g is rows rows_host[offsets_host[g] .. offsets_host[g + 1]) of emb (n x d; repeats allowed, offsets_host[0] == 0, n_groups + 1
 * offsets).  normalize_rows != 0: every gathered row is divided by its L2 norm (whitebox.py:778-783), the rows are averaged and the mean is divided
 * by its norm (filter_inpaintinggame_for_net.py:107-109,143-146; plot_inpainting_game.py:934-943).  normalize_rows == 0: the rows are summed and the
 * sum is divided by its norm (eccv20.py:53-54).  Norms and sums in float64, every stored value rounded once.  out_dev: n_groups x d. */
xfr_status XFR_EX xfr_embed_templates(xfr_engine* e, const float* emb_dev, int32_t n, int32_t d, const int32_t* rows_host, const int32_t* offsets_host,
                                      int32_t n_groups, int32_t normalize_rows, float* out_dev, void* stream);
/* out_dev[p] = |A[i_p] - B[j_p]| for the n_pairs pairs (i_p, j_p) = (pairs_host[2 p], pairs_host[2 p + 1]); A is na x d, B is nb x d and may be A
 * (net_mate_nonmate_dists.py:127-128, filter_inpaintinggame_for_net.py:114,149,164-165). */
xfr_status XFR_EX xfr_pair_dists(xfr_engine* e, const float* a_dev, int32_t na, const float* b_dev, int32_t nb, int32_t d, const int32_t* pairs_host,
                                 int32_t n_pairs, float* out_dev, void* stream);
/* The k nearest rows of the gallery (ng x d) to every query (nq x d; may be the gallery itself): idx_dev int32 nq x k and dist_dev float32 nq x k in
 * increasing distance, equal float32 distances by lower gallery index -- squareform(pdist(X)) and argsort of every row (eccv20.py:57-59) without the
 * nq x ng matrix.  exclude_same_index != 0: query i ignores gallery row i, the reference's dropped self distance (:58). */
xfr_status XFR_EX xfr_nearest_rows(xfr_engine* e, const float* q_dev, int32_t nq, const float* g_dev, int32_t ng, int32_t d, int32_t k,
                                   int32_t exclude_same_index, int32_t* idx_dev, float* dist_dev, void* stream);

/* ---- Saliency finishing (python/xfr/show.py:196-222 create_save_smap, :131-137 processSaliency, :46-129 blend_saliency_map).  An additive entry
 * point, ABI version 7. -----------------------------------------------------------------------------------------------------------------------
 * What the generator does to every map between producing it and storing it, for n float32 maps of h x w and probes of out_h x out_w:
 *     float32 head     s = m - min(m);  total = the float32 nearest to the sum of s, accumulated in float64 in a fixed order (totals_host[i] instead,
 *                      where given: numpy's own float32 sum);  s = s / total, a correctly rounded float32 quotient.  total == 0 (a constant map)
 *                      gives the all-zero map; numpy's 0 / 0 makes it NaN
 *     normalise        a = (double)s - min;  a = a / (max + 1e-9)
 *     resize           scipy.ndimage.zoom(a, order=3, mode='grid-constant', cval=0, grid_mode=True) in closed form -- 12 zeros on every side, the
 *                      B-spline prefilter with pole sqrt(3) - 2 along axis 0 then axis 1, 16 taps at x = (o + 0.5) (in / out) - 0.5 + 12 -- clipped
 *                      to [min(a.min, 0), max(a.max, 0)].  out_h x out_w == h x w: a itself, bit for bit
 *     overlay          only with probes (uint8, n x out_h x out_w x 3, img = k / 255.0): att = v - min(v) over the finished map; max(att) <= 0: the
 *                      image; else att /= max, alpha = att^0.8, colour = table[min(int(att * 256), 255)] (255 at att >= 1), and the byte is
 *                      uint8(clip((1 - alpha) img + alpha colour, 0, 1) * 255), truncated.  jet_lut_host: the 256 x 3 float64 table, HOST memory
 * Float64 throughout behind the head, no operation contracted; a map's bits depend on the map alone, not on n, its place in the batch or the launch.
 * maps_dev, probes_u8_dev and the outputs are on the engine's device; totals_host and jet_lut_host are read before the call returns; the work is
 * enqueued on `stream`.  The engine lends its device and its error text and owns the call's workspace: no weights are needed.
 * XFR_INVALID_ARG before anything is launched, with a text naming the value: a null engine, maps or sal_out_dev; n outside [1, XFR_FINISH_MAX_MAPS];
 * an axis outside [1, XFR_FINISH_MAX_DIM]; a shrinking axis (out < in: the Gaussian pre-filter path stays on the host); an output size the zoom's
 * own rounding would not produce; probes without a table or without overlay_out_dev, or an overlay output without probes; a total that is negative
 * or not finite; buffers that overlap (by the sizes the counts imply). */
#define XFR_FINISH_MAX_MAPS 65535
#define XFR_FINISH_MAX_DIM 4096
xfr_status XFR_EX xfr_finish_saliency(xfr_engine* e, const float* maps_dev, int32_t n, int32_t h, int32_t w, int32_t out_h, int32_t out_w,
                                      const float* totals_host, const uint8_t* probes_u8_dev, const double* jet_lut_host, double* sal_out_dev,
                                      uint8_t* overlay_out_dev, void* stream);

/* ---- Image intake (python/xfr/models/whitebox.py:787-806 convert_from_numpy behind python/xfr/utils.py:39-202 image_loader).  Additive entry
 * points, ABI version 7. -----------------------------------------------------------------------------------------------------------------------
 * From decoded uint8 crops of unequal sizes to the network-size uint8 batch that xfr_forward_u8 and xfr_triplet_contrastive_u8[_host] take.  For
 * a crop u of h x w x channels bytes (rows row_stride bytes apart, the first at `offset` of the source buffer) and an output of out_h x out_w:
 *     head        XFR_INTAKE_HEAD_F64 (files, DataFrame rows): a = (double)u / 255.0;  XFR_INTAKE_HEAD_F32 (uint8 arrays handed to
 *                 convert_from_numpy): a = (double)((float)u / 255.0f)
 *     same size   h x w == out_h x out_w: no resize, the byte is uint8(a * 255.0), in float32 up to the truncation under the F32 head
 *     pre-filter  only on an axis whose factor f = in / out exceeds 1, axis 0 then axis 1: scipy.ndimage.gaussian_filter(mode='mirror'),
 *                 sigma = (f - 1) / 2 (no pass at sigma <= 1e-15), radius int(4 sigma + 0.5), weights exp(-0.5 / sigma^2 x^2) / their sum, summed
 *                 from the outermost pair inwards around the centre term
 *     zoom        scipy.ndimage.zoom(order=1, mode='mirror', grid_mode=True): cc = (o + 0.5) (in / out) - 0.5, c = |cc|, taps floor(c) and the
 *                 next, mirrored at the far edge, weights 1 - (c - floor(c)) and its complement, the four products added row by row
 *     clip, byte  clipped to [min a, max a] over all channels of the crop (alpha included), then uint8(v * 255.0), truncated
 *     channels    one channel is replicated to three, a fourth is dropped (PIL's convert('RGB'))
 *     tap tables  row_tab (final_h entries over out_h) and col_tab (final_w entries over out_w), both or neither, HOST memory: Pillow's integer
 *                 bilinear resize and crop of those bytes, the horizontal pass first and rounded to uint8 (lightcnn.py:27-31 Resize + CenterCrop;
 *                 the entries are those of xfr_strise_options).  final_h and final_w are ignored without tables
 * out_dev is n x out_h x out_w x 3 bytes, or n x final_h x final_w x 3 with tables.  Float64 throughout, no operation contracted, one thread per
 * output element: a crop's bytes depend on the crop alone, not on n, its place in the batch or the launch.  They equal the host chain's
 * (saliency_io.resize_linear + truncation) byte for byte given the same Gaussian weights; the weights are libm's exp under numpy's summation, or the
 * caller's own where xfr_intake_set_kernels states them (numpy's vectorised exp differs from libm's in the last bit of about one weight in twenty).
 * The engine lends its device, its error text, its copy stream and the workspace (at most 512 MB of pre-filter planes per chunk of crops, more
 * only for a single crop that needs it): no weights are needed and n is not bound by max_batch.  The work is enqueued on `stream`; items_host and
 * the tables are read before the call returns.
 * xfr_intake_u8_host: the same for a source in HOST memory, read before the call returns: copied to pinned memory, uploaded on the engine's copy
 * stream, and `stream` waits for that upload alone.
 * XFR_INVALID_ARG before anything is launched, with a text naming the value: a null engine, source, items or output; n outside
 * [1, XFR_INTAKE_MAX_ITEMS]; channels outside {1, 3, 4}; an unknown head; an axis of a crop, of the output or of the final size outside
 * [1, XFR_INTAKE_MAX_DIM]; a row stride shorter than a row; an item that leaves [0, src_bytes); a pre-filter radius above XFR_INTAKE_MAX_RADIUS
 * (64: factors up to 33.1); an output size the zoom's own rounding, round(in * (1 / (in / out))), would not produce; one table without the other;
 * table entries xfr_strise_score_ex would refuse; an output that overlaps the source. */
#define XFR_INTAKE_MAX_ITEMS 65535
#define XFR_INTAKE_MAX_DIM 4096
#define XFR_INTAKE_MAX_RADIUS 64
enum { XFR_INTAKE_HEAD_F64 = 0, XFR_INTAKE_HEAD_F32 = 1 };
typedef struct {
    int64_t offset;                     /* the crop's first byte in the source buffer */
    int32_t h, w, row_stride, channels, head;
} xfr_intake_item;
xfr_status XFR_EX xfr_intake_u8(xfr_engine* e, const uint8_t* src_dev, size_t src_bytes, const xfr_intake_item* items_host, int32_t n, int32_t out_h,
                                int32_t out_w, const xfr_strise_tap* row_tab, const xfr_strise_tap* col_tab, int32_t final_h, int32_t final_w,
                                uint8_t* out_dev, void* stream);
xfr_status XFR_EX xfr_intake_u8_host(xfr_engine* e, const uint8_t* src_host, size_t src_bytes, const xfr_intake_item* items_host, int32_t n,
                                     int32_t out_h, int32_t out_w, const xfr_strise_tap* row_tab, const xfr_strise_tap* col_tab, int32_t final_h,
                                     int32_t final_w, uint8_t* out_dev, void* stream);
/* The caller's own Gaussian kernels for the pre-filter, replacing those stated before (count 0: none): kernel i serves every axis whose sigma and
 * radius are exactly sigmas_host[i] and radii_host[i]; weights_host is count x (XFR_INTAKE_MAX_RADIUS + 1) doubles, row i holding the normalised
 * weights of x = -radius .. 0.  A Python caller states numpy's kernels here so that the bytes equal scipy's on any host. */
xfr_status XFR_EX xfr_intake_set_kernels(xfr_engine* e, const double* sigmas_host, const int32_t* radii_host, const double* weights_host, int32_t count);

/* Debug / parity: after an xfr_ebp call made while tracing is enabled, the per-firing trace
 * sum(P[i]) (what the golden fixtures store for every entry of Whitebox.P, whitebox.py:394).
 * xfr_engine_set_trace(e, 1) makes xfr_ebp record it (slower).  `sums` receives n_firings x S x N doubles
 * in the reference's firing order; `kinds` (may be NULL) receives the xfr_op_kind of the hooked module. */
xfr_status xfr_engine_set_trace(xfr_engine* e, int32_t enable);
xfr_status xfr_engine_trace_size(xfr_engine* e, int32_t* n_firings);
xfr_status xfr_engine_get_trace(xfr_engine* e, double* sums, int32_t* kinds, int32_t capacity);

/* Test hook: the tail of xfr_contrastive_raw -- the per-sample sums, the truncation threshold, the contrast; no blur -- on a tensor the caller
 * supplies, by exactly the launches the engine makes on its own P[-2].  Additive entry point, ABI version 7.
 *   p_dev         [c][2 n][hw] float32, the engine's internal channel-major layout: rows 0 .. n-1 the mate sweep, n .. 2n-1 the non-mate sweep
 *   percentile    0 .. 100: keep m = P / S where m >= the threshold (whitebox.py:550-556); below 0: the plain contrastive form (:524-526) -- no
 *                 threshold launches, thr_dev is not written
 *   sums_dev      NULL, or 2 n doubles: the sums S of the 2 n rows over c and hw
 *   thr_dev       NULL, or n floats: the threshold of every sample, the smallest kept value of m
 *   contrast_dev  n x hw float32
 * The engine lends its device and its error text: no weights are needed and n is not bound by max_batch.  The call allocates its own scratch,
 * enqueues on `stream`, WAITS for the stream and frees the scratch: it is a hook for tests, not for a hot path.
 * XFR_INVALID_ARG before anything is launched, with a text naming the value: a null e, p_dev or contrast_dev; c, n or hw below 1 (2 n above 65535);
 * a percentile above 100 or NaN; an output that overlaps p_dev (by the sizes the counts imply); a p_dev that is not 16-byte aligned (the sums read
 * float4 whenever hw % 4 == 0, as they may on the engine's own aligned workspace). */
xfr_status XFR_EX xfr_debug_contrast_tail(xfr_engine* e, const float* p_dev, int32_t c, int32_t n, int32_t hw, float percentile, double* sums_dev,
                                          float* thr_dev, float* contrast_dev, void* stream);

/* Test / tuning hook: one forward convolution through the engine's implicit-GEMM kernel, outside any engine.
 * in_dev/out_dev are CNHW device tensors ([C][NB][H][W]); w_host/bias_host are PyTorch-layout host arrays.
 * cfg % 100: 0 lets the launcher pick the tile configuration, 4 / 5 force the 16- / 32-deep 64x64 configuration;
 * (cfg / 10000) % 100: tail balancing 0 = heuristic, 1 = off, S >= 2 = S parts per tail tile; cfg / 1000000 = n in 2..4: the
 * launches go to n streams at once (aggregate rate of co-running launches; *ms_out is then the time per launch).
 * (cfg / 100) % 10 == 1: the lean probe-forward launch of a convolution behind BatchNorm (scale 1, shift 0) + ReLU -- the W and relu(W)
 * tiles in one workgroup; the input must be non-negative (relu_in 0), nb * OH * OW a multiple of 4, and out_dev holds TWO tensors:
 * relu(conv(W) + b), then q = relu(conv(W) + b) / (relu(conv(relu W) + b) + 1e-16) with its sign bit set where the first is <= 0.  The kernel is run
 * `reps` times after one untimed launch; *ms_out receives the average duration (HIP events on the null stream). */
xfr_status xfr_debug_conv(const float* in_dev, const float* w_host, const float* bias_host, float* out_dev, int32_t cin,
                          int32_t h, int32_t w, int32_t nb, int32_t cout, int32_t kh, int32_t kw, int32_t stride,
                          int32_t pad, int32_t relu_in, int32_t cfg, int32_t reps, float* ms_out);

/* Test hook: ONE grouped-convolution launch (Conv2d(groups = G): configuration 13, the grouped MFMA kernel, or 14, the depthwise kernel) outside any
 * engine, on the caller's pointers as the engine's forward, backward-data and phase launches make them.  Additive entry point, ABI version 7.
 *   in_dev               [cin][in_nb][h][w] float32; the first nb images of every channel are read
 *   out0_dev, out1_dev   [cout][out_nb][out_H][out_W]; the first nb images are written.  The pointers are taken as they come: a caller that wants
 *                        a phase's pre-offset target, or a pointer that is not 16-byte aligned, passes it so.  out1_dev: the relu(W) half, read only
 *                        when nhalves == 2
 *   w_host               [cout][cin / groups][kh][kw], PyTorch's layout; the call builds the per-group pack and, for nhalves == 2, the pack of
 *                        max(w, 0).  A backward-data or phase launch is a forward launch to the kernels: its caller prepares the flipped,
 *                        transposed or phase-sliced weight
 *   bias_host, bias_pos_host   NULL or cout floats, added to out0 / out1
 *   pad, pad_dw          rows are padded by pad, columns by pad + pad_dw on both sides: OH = (h + 2 pad - kh) / stride + 1,
 *                        OW = (w + 2 (pad + pad_dw) - kw) / stride + 1, M = nb OH OW, K = cin / groups * kh * kw
 *   accumulate           1: out += result
 *   out_stride, out_H, out_W   output (oh, ow) lands at (oh out_stride, ow out_stride) of an out_H x out_W map; out_H = out_W = 0: the dense
 *                        OH x OW map (out_stride 1)
 *   cfg                  13: the grouped kernel; 14: the depthwise kernel, XFR_UNSUPPORTED_LAYER with nothing launched where it does not take the
 *                        launch; 0: as the engine picks -- the depthwise kernel where it takes the launch, else the grouped one
 *   cfg_out, tile_out    NULL, or where the configuration that ran and the depthwise kernel's tile (outputs per workgroup; 0 for configuration 13) go
 * One launch on the null stream, then the call WAITS for it; nothing is timed.  XFR_INVALID_ARG before any device call, with a text naming the
 * values: a null in_dev, out0_dev or w_host; nhalves outside 1 .. 2 or two halves without out1_dev; a cfg other than 0, 13, 14; fewer than two
 * groups or groups that do not divide cin and cout; a size, tap count or stride below 1; nb below 1 or above in_nb or out_nb; flags other than 0 / 1;
 * padding that leaves no output; a target map that does not hold the strided outputs; a tensor of 2^31 elements or more. */
xfr_status XFR_EX xfr_debug_conv_grouped(const float* in_dev, float* out0_dev, float* out1_dev, const float* w_host, const float* bias_host,
                                         const float* bias_pos_host, int32_t cin, int32_t cout, int32_t groups, int32_t h, int32_t w, int32_t nb,
                                         int32_t in_nb, int32_t out_nb, int32_t kh, int32_t kw, int32_t stride, int32_t pad, int32_t pad_dw,
                                         int32_t relu_in, int32_t nhalves, int32_t accumulate, int32_t out_stride, int32_t out_H, int32_t out_W,
                                         int32_t cfg, int32_t* cfg_out, int32_t* tile_out);

/* Tuning hook: while stamps_dev is non-NULL, every GEMM launch of this process records, per wave, 8 64-bit words at
 * stamps_dev[(block * 4 + wave) * 8]: s_memrealtime (100 MHz) at kernel entry / first operands landed / K loop done / epilogue entered / exit,
 * then HW_ID, XCC_ID, and the wave's life in shader-clock cycles (s_memtime; with the 100 MHz stamps: the effective clock) (tools/conv_sweep.py --stamps draws a launch's timeline from them).  The buffer holds
 * 32 words for each of capacity_workgroups workgroups; workgroups beyond that do not record.  NULL switches it off (the default).
 * capacity_workgroups < 0: sampled mode for whole steps (tools/phase_probe.py) -- the buffer holds -capacity_workgroups records in regions
 * of 256; the n-th launch writes up to 256 evenly spaced workgroups into region n % regions, word 6 also carries K, M and Cout of the launch. */
xfr_status xfr_debug_conv_stamps(void* stamps_dev, int32_t capacity_workgroups);

/* Tuning hook: a timeline of the GEMM launches as the device ran them, streams overlapped.  While log_dev is non-NULL (zero-filled
 * device memory, 64 bytes per launch, `capacity` launches), every GEMM launch of this process records when its first workgroup
 * started and its last one ended (s_memrealtime, 10 ns ticks) and the library notes its shape, stream and tile configuration.  A
 * call with dump_path != NULL first writes what has been recorded so far as CSV (synchronise the device before); log_dev = NULL
 * stops recording.  tools/gemm_timeline.py reads the file.  (The launches of grouped convolutions -- configuration 13, their own kernel -- are not in
 * this log; the profile records of xfr_engine_profile_csv list them.)
 * xfr_debug_conv_stamps and xfr_debug_conv_log are PROCESS-GLOBAL (every engine of the process records into them) and mutex-guarded: engines
 * may launch from other host threads while they are set, dumped or cleared; launches only touch the lock while a hook is on.  A dump after
 * log_dev = NULL writes nothing and returns XFR_OK. */
xfr_status xfr_debug_conv_log(void* log_dev, int32_t capacity, const char* dump_path);

/* Bytes of device memory held by the engine (weights + workspace). */
xfr_status xfr_engine_memory(xfr_engine* e, size_t* weight_bytes, size_t* workspace_bytes);

/* Duration in ms of the conv/linear GEMM launches of the most recent run call (sum of HIP-event timings on the
 * run's stream) and their count and algorithmic FLOPs; enabled by xfr_engine_set_profile(e, 1).  Used by
 * bench.py for the live roofline figure. */
xfr_status xfr_engine_set_profile(xfr_engine* e, int32_t enable);
xfr_status xfr_engine_get_profile(xfr_engine* e, double* gemm_ms, int64_t* gemm_launches, double* gemm_flops);
/* The same three figures split by the kernel family that really ran each launch (ABI version 6): index 0 the fp32 MFMA kernels, index 1 the bf16x6
 * kernel -- each family has its own ceiling (157.3 / 419.4 fp32-equivalent TFLOP/s), and bench.py reports a roofline fraction per family.  Arrays of 2. */
xfr_status xfr_engine_get_profile_by_kernel(xfr_engine* e, double* gemm_ms, int64_t* gemm_launches, double* gemm_flops);
/* While profiling is on, also append one CSV record per GEMM launch to `path` (NULL: stop):
 * Cout,nhalves,K,M,kh,stride,out_stride,relu_in,accumulate,ms,TFLOP/s,cfg  (profiles/layer_table.py reads it; cfg = the configuration that ran, 9 = bf16x6,
 * 13 = the grouped-convolution kernel, whose K is that of one group: Cin / groups * kh * kw). */
xfr_status xfr_engine_profile_csv(xfr_engine* e, const char* path);

/* Process-wide counts of GEMM launches that carried a fused elementwise chain: those whose epilogue was one of the
 * compile-time specialised ones (xfr_amd/csrc/chain_sigs.inc) and those that fell back to the interpreter; n_signatures =
 * size of the compiled table.  bench.py snapshots the counters right after its timed loop and fails `outputs_ok` if an interpreted
 * launch ran there; tests/test_gpu_entry.py asserts interpreted == 0 for the benchmarked entry point on the BASELINE backbones. */
xfr_status xfr_chain_epilogue_stats(int64_t* compiled_launches, int64_t* interpreted_launches, int32_t* n_signatures);

/* Process-wide launch counts of the kernel variants that the pool, normalize, direct-stem and hook-chain launchers choose between by shape and
 * pointer alignment (the scalar kernels, the float4 ones, the row-pair max-pools, the fused pool pair, the global average pool; the chain kernels
 * by interpreter and by chain head).  Counted on the host where a kernel is enqueued: the planner and the dry run of the lean schedule count
 * nothing.  xfr_elementwise_variant_name(i) names variant i, NULL beyond the last; `counts` receives min(capacity, n_variants) values in that
 * order and `n_variants` (may be NULL) their number.  No device needed.  tests/test_gpu_layer_parity.py proves with them that each variant ran
 * under a float64 comparison. */
xfr_status xfr_elementwise_launch_stats(int64_t* counts, int32_t capacity, int32_t* n_variants);
const char* xfr_elementwise_variant_name(int32_t i);

/* The planner without a device: the fused forward-only and backward schedules of a layer program for one subtree mode and
 * seed tensor, as text (one launch per line; GEMM lines carry the signature of their fused chain and the index of its
 * compiled epilogue, -1 if it would be interpreted).  Makes no HIP call, so it also runs where no GPU is visible:
 * tools/gen_chain_sigs.py builds chain_sigs.inc from it and the CPU test-suite checks the table against it.
 * `needed` (may be NULL) receives the full length including the terminator; `buf` gets at most `capacity` bytes. */
xfr_status xfr_plan_describe(const xfr_op_desc* ops, int32_t n_ops, int32_t n_weights, int32_t in_c, int32_t in_h, int32_t in_w,
                             int32_t batch, int32_t subtree_mode, int32_t seed_tensor, char* buf, size_t capacity, size_t* needed);

#ifdef __cplusplus
}
#endif
#endif /* XFR_AMD_H */
