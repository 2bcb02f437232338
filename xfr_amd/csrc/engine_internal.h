// engine_internal.h -- what the host translation units of the engine share: the planner's records (Hook, Tensor, OpRec, BwdStep, BwdPlan), the engine
// object, the families' state objects and the functions that cross files.  Nothing here is part of the C ABI (include/xfr_amd.h).
//   plan.hip           shape inference, hook table, workspace / arena layout, the un-fused backward schedule (device-free)
//   plan_fuse.hip      the fusion passes over that schedule and the lean rewrite (device-free)
//   forward.hip        forward fusers and the forward executor
//   backward.hip       chain resolution and the sweep executor
//   hip_owner.h        the error helpers and the owners of device buffers, pinned buffers, events and streams (included here)
//   scoped.h           Scoped<T>: a value written for the length of a scope, the one guard of these files (included here)
//   engine.hip         the C ABI: create / destroy / weights / setters / forward / EBP / contrastive / triplet / uint8 / profiling
//   weights.hip        the packs of the weight arena, filled on the host; the bf16 planes of the covered packs
//   debug_abi.hip      the C ABI: the xfr_debug_* entry points
//   subtree.hip        the C ABI: layerwise and weighted-subtree EBP
//   probe_sweep.hip    the batched sweep with its side stream that the next two share (ProbeSweep)
//   strise_abi.hip     the C ABI: STRise blackbox saliency
//   inpaint_abi.hip    the C ABI: inpainting-game scoring
//   match_abi.hip      the C ABI: match calibration (templates, pair distances, nearest rows)
//   finish_abi.hip     the C ABI: saliency finishing (normalise, spline resize, jet overlay)
//   intake_abi.hip     the C ABI: image intake (crop, Gaussian pre-filter, linear resize, bytes)
//   comm.hip           the C ABI: the RCCL binding
//   plan_describe.hip  the C ABI: xfr_plan_describe
#pragma once
#include "../../include/xfr_amd.h"
#include "common.h"
#include "hip_owner.h"
#include "scoped.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <memory>
#include <string>
#include <vector>

namespace xfr {

enum PState { PS_EQ = 0, PS_RELU = 1, PS_OTHER = 2 };

struct Hook {
    int op;        // hooked module call
    int j;         // which input of that call
    int a_tensor;  // tensor providing a (and x): the LAST input of the call (whitebox.py:379-381 late binding)
};

struct Tensor {
    int C = 0, H = 0, W = 0;
    int producer = -1;
    std::vector<int> consumers;
    bool nonneg = false;
    int pstate = PS_OTHER;
    int alias = -1;          // shares T storage with this tensor (in-place ReLU, Split)
    int prefix_of = -1;      // T storage = the leading channels of this tensor's (the pooled shortcut inside its zero-padded form; layout_workspace)
    size_t t_off = 0, pv_off = 0, g_off = 0;   // offsets (floats) into the workspace
    bool need_pv = false;
    std::vector<Hook> hooks;
    long per_n() const { return (long)C * H * W; }
    int HW() const { return H * W; }
};

// One phase of the backward-data pass of a strided KxK convolution (stride s, padding p): the input pixels with ((ih + p) % s, (iw + p) % s) == (r, c)
// see only the taps a = r, r + s, ... < kh and b = c, c + s, ... < kw, and their gradient is an ordinary stride-1 convolution of dY with the flipped
// ka x kb sub-kernel (top / left padding ka - 1 - q0 / kb - 1 - u0), whose nq x nu results land at dX[ih0 + s i][iw0 + s j].
struct PhaseRec {
    int r = 0, c = 0;
    int ka = 0, kb = 0;        // taps of the phase per axis: ceil((kh - r) / s), ceil((kw - c) / s)
    int q0 = 0, u0 = 0;        // first output row / column of the forward whose window holds a pixel of the phase: max(0, ceil((p - r) / s))
    int ih0 = 0, iw0 = 0;      // the phase's first input pixel: s q0 + r - p
    int nq = 0, nu = 0;        // the phase's pixels per axis: (H - 1 - ih0) / s + 1
    int K = 0;                 // cout * ka * kb (of one group: cout / groups * ka * kb)
    bool tap = false;          // K packed tap-major (tap, co)
    long w_bwd = -1, w_bwd_true = -1;      // the phase's relu(W) and true packs in the arena
};

struct OpRec {
    xfr_op_desc d;
    std::vector<PhaseRec> phases;            // a strided KxK convolution behind the first layer: the launches of its backward-data pass (layout_arena)
    // packed parameter offsets (floats) into the arena; -1 if absent
    long w_true = -1, w_pos = -1, w_bwd = -1, w_bwd_true = -1;   // w_bwd_true: true-weight backward pack (plain gradients)
    long b_true = -1, b_pos = -1;            // conv/linear bias and relu(bias)
    long bn_alpha_t = -1, bn_beta_t = -1, bn_alpha_p = -1, bn_beta_p = -1, bn_beta_pb = -1;
    int ldw = 0, ldb = 0;
    bool tap_fwd = false, tap_bwd = false;   // K packed tap-major (kh,kw,ci) for the forward / backward-data GEMM
    bool tap4_fwd = false;                   // image stems (Cin 3 or 4): K packed (kh,kw,4 channel slots); Kf = rows of the forward pack
    int Kf = 0;
    int Cin = 0, K = 0, Kb = 0;
    int groups = 1;                          // > 1: a grouped convolution (xfr_op_desc::ceil_mode of a CONV).  K, Kb and PhaseRec::K are then those of ONE group
                                             // (Cin / groups * kh * kw, cout / groups * kh * kw), the packs per group (conv_group.hip), and the layer carries
                                             // no fused chain, no lean rewrite, no bf16x6, no tail balancing, no pair_m and no as_strided form
    size_t idx_off = 0;                      // maxpool argmax (bytes into idx workspace)
    size_t norm_off = 0;                     // normalize: norms (floats into misc workspace)
    int pair = 0;                            // MaxFeatureMap convolution (Conv -> Split -> max of halves, lightcnn.py:48-62): Co = cout / 2; its forward
                                             // pack (and bias) holds the output channels interleaved (column 2c = channel c, 2c+1 = channel c + Co)
    int pair_split = -1, pair_max = -1;      // the Split and G_MAXHALVES ops behind it
    bool fuse_relu = false;                  // forward: the following in-place ReLU is applied in this op's kernel
    bool relu_fused_away = false;            // forward: this ReLU is executed by its producer
};

enum StepKind { ST_EW, ST_CONV_BWD, ST_MAXPOOL_BWD, ST_AVGPOOL_BWD, ST_COPY, ST_MAXHALVES_BWD, ST_NORMALIZE_BWD, ST_ZERO };


struct BwdStep {
    int kind;
    int op = -1;
    int src_t = -1, dst_t = -1;
    int accumulate = 0;
    long copy_elems_per_sb = 0;   // ST_COPY: channels to copy (prefix), dst/src channel counts differ for concat
    // ST_EW: symbolic chain (resolved to pointers at run time)
    struct Sym { int type; int action; int t0; int x_t; float f; int op; int slot; bool tap; };
    std::vector<Sym> chain;   // ST_EW: the chain; ST_CONV_BWD: epilogue chain fused into the GEMM (may be empty)
    int ew_t = -1;     // tensor whose shape the chain runs over
    bool compact = false;   // ST_CONV_BWD of a 1x1 / stride 2 convolution: the result stays on the sampled grid, dense, at the start of dst_t's gradient
                            // region (the chain head EW_AVGUP_IN of the launch that follows puts it in place)
};

struct BwdPlan {
    int seed_tensor = -1;
    int mode = -1;
    bool plain = false;              // true-weight gradients without hooks (whitebox.py:652-676 dA lists)
    std::vector<int> firing_tensor;  // tensor whose gradient each firing sees
    std::vector<BwdStep> steps;      // one launch per step, no cross-kernel fusion (used when tracing)
    std::vector<BwdStep> fused;      // after copy forwarding and chain -> chain merging
    std::vector<BwdStep> fused_gemm; // ... and with the chains that follow a backward GEMM run in its epilogue
    std::vector<BwdStep> fused_gemm_nofan; // the same without the MaxFeatureMap fan-out (a compiled-only epilogue step): what the interpreted epilogues run
    std::vector<int> firing_kinds;   // xfr_op_kind per firing, reference order
    std::vector<int> firing_ops;     // hooked module call (op index) per firing: Whitebox.P_layername is str(module) of these (whitebox.py:393)
    int n_firings = 0;
    int fan_ok = -1;                 // does every fan-out epilogue of fused_gemm have a compiled signature (-1: not checked yet; fanout_compiled)
    // The lean schedule (xfr_engine_set_lean): the probe forward stores quotients instead of hook operands, the sweep reads them.
    int lean_state = -1;             // -1 not prepared, 0 does not apply to this plan, 1 ready (lean_prepare)
    std::vector<char> lean_q;        // per tensor: 1 = its T storage holds a / (x + eps) of the BatchNorm hook on it (sign bit: lean_final <= 0),
                                     // 2 = its Pv storage holds a / (x + eps) of the in-place ReLU hook behind it
    std::vector<int> lean_final;     // per tensor with lean_q 1: root of the tensor whose positivity the sign bit records (-1: none)
    std::vector<BwdStep> fused_gemm_lean;
};

}  // namespace xfr
using namespace xfr;

// xfr_strise_* and xfr_inpaint_*: what their sweeps share, one per engine (probe_sweep.hip)
struct ProbeSweep {
    Stream s_gen;                                      // the images of batch i + 1 are built here while batch i encodes
    Event ev_in, ev_ready[2], ev_free[2];
    Event ev_done;                                     // the end of the previous call of either family, on that call's stream
    bool done_recorded = false;
    DevBuf<float> xbuf[2];                             // two batches of network input, max_batch x in_c x in_h x in_w
    DevBuf<float> emb;                                 // max_batch x D embeddings of the running batch
};

// The families' own buffers, one object per engine, built on first use.  Every member is an owner: the object goes with the engine.
struct StriseState {                                   // xfr_strise_* (strise_abi.hip)
    DevBuf<double> orig;                               // n_refs + n_gal similarities of the unmasked probe, then as many 1 / |g|
    DevBuf<int> tab;                                   // cells, shifts, shift order and group offsets of the current call
    DevBuf<double> merge_ws;                           // A [scale^2][gh * gw] and wsum [scale^2]
};

struct InpaintState {                                  // xfr_inpaint_* (inpaint_abi.hip)
    DevBuf<char> scratch;                              // per map: the sort's keys, indices and running sums
    DevBuf<uint8_t> first_on;                          // n_maps x H x W
};

struct MatchState {                                    // xfr_embed_templates / xfr_pair_dists (match_abi.hip)
    Event ev_done;                                     // the end of the previous call, on that call's stream: its kernels read `tab`
    bool done_recorded = false;
    DevBuf<int> tab;                                   // the index table of the running call
};

struct FinishState {                                   // xfr_finish_saliency (finish_abi.hip)
    Event ev_done;                                     // the end of the previous call, on that call's stream: its kernels read all of the below
    bool done_recorded = false;
    DevBuf<double> planes;                             // the padded coefficient planes of the running call's maps
    DevBuf<double> stats;                              // FINISH_STATS doubles per map
    DevBuf<float> totals;                              // the caller's totals
    DevBuf<double> lut;                                // the colour table, uploaded when it differs from lut_host
    double lut_host[768];
    bool lut_set = false;
};

struct IntakeKernel { double sigma; int radius; double w[INTAKE_WEIGHTS]; };      // w[0 .. radius], w[radius] the centre

struct IntakeState {                                   // xfr_intake_u8[_host] (intake_abi.hip)
    Event ev_done;                                     // the end of the previous call, on that call's stream: its kernels read all of the below
    Event ev_copied;                                   // the end of the previous upload on the engine's copy stream
    bool done_recorded = false, copied_recorded = false;
    DevBuf<IntakeItem> items;                          // the running call's crops
    DevBuf<double> wts;                                // [n][2][INTAKE_WEIGHTS]
    DevBuf<double> lohi;                               // [n][2]
    DevBuf<double> plane_a, plane_b;                   // the pre-filter's two planes of a chunk
    DevBuf<uint8_t> q, mid;                            // with tap tables: the zoom's bytes, then the horizontal pass's
    DevBuf<StriseTap> taps;                            // row table, then column table
    DevBuf<uint8_t> stage_dev;                         // xfr_intake_u8_host: the sources on the device ...
    PinnedBuf<uint8_t> stage_host;                     // ... and in pinned host memory on their way there
    std::vector<IntakeKernel> stated;                  // the caller's own kernels (xfr_intake_set_kernels)
};

// the side streams on which the phases of one strided KxK layer's backward-data pass run next to the sweep's own stream: one all-or-nothing group
struct PhaseStreams {
    Stream s[3];
    Event fork, done[3];
};

// What one sweep needs beyond its plan, as a value: the entry point that observes a sweep (priors, captures, a stored firing, ascending prefixes; subtree.hip)
// builds one on its stack and hands it down; nothing of it lives on the engine.  A default-constructed one is the plain sweep.
struct SweepCtx {
    bool priors = false, caps = false;                // are the priors / the captures of this call live?
    std::vector<char> prior_row, cap_row;             // per firing: does the row of the tables hold any entry?
    int dense_slot = -1;                              // firing that carries the dense prior (-1: none) ...
    const float* prior_dense = nullptr;               // ... and that tensor (single sweep of one image)
    int store_slot = -1;                              // firing whose full P tensor is kept (-1: none) ...
    float* store_dst = nullptr;                       // ... and where
    // the tables [n_firings][tab_sb] over the gradient rows sb (stream * n + sample), on the device (common.h: EwStep::prior_elem / cap_elem)
    const int* tab_elem = nullptr;                    // prior element (or capture element) per (firing, row); -1: none
    const float* tab_val = nullptr;                   // prior value per (firing, row)
    float* cap_dst = nullptr;                         // captured value per (firing, row)
    int tab_sb = 0;                                   // their row length
    std::vector<int> active;                          // layerwise sweeps in ascending firing order: stream j (all its samples) is identically zero before firing active[j]
    int n = 1;                                        // samples per stream of that batch
    bool lazy_zero = false;                           // prefix sweeps: run_backward zeroes un-written gradient rows on demand (xfr_layerwise_ebp)
    bool observing() const { return priors || caps || store_slot >= 0; }      // such a sweep keeps its chains in launches of their own, and never runs lean
};

struct xfr_engine {
    // ---- geometry: the network, its plans and the layout of the workspace (plan.hip)
    int device = 0;
    int max_batch = 0;
    int in_c = 0, in_h = 0, in_w = 0;
    std::vector<OpRec> ops;
    std::vector<Tensor> tens;
    int n_weights = 0;
    std::vector<char> is_hook_a;       // per tensor: some hook takes its a (and x) from this tensor's forward values
    bool need_dirty = true;
    std::deque<BwdPlan> plans;         // deque: get_plan() hands out pointers that must survive later insertions
    size_t arena_floats = 0, ws_floats = 0, idx_bytes = 0;
    size_t x_off = 0, seed_off = 0, tap_off = 0, pooled_off = 0, blur_a_off = 0, blur_b_off = 0, misc_off = 0, thr_off = 0;
    size_t g_begin = 0, g_end = 0;                    // the gradient region of the workspace (floats)
    size_t t_region_floats = 0, fwd_region_floats = 0;
    size_t trace_cap = 0;          // firings capacity
    // ---- streams and events.  They come first: members go in reverse order, so every buffer below is freed before the streams and events it was used on.
    Stream s_a, s_b;                   // the two internal streams, with ev_fork / ev_a / ev_b one all-or-nothing group (ensure_streams)
    Event ev_fork, ev_a, ev_b;
    // xfr_triplet_contrastive_u8_host: the engine's own copy stream and one uint8 staging buffer per forward slot -- fresh inputs keep the cross-call overlap
    Stream s_copy;
    Event ev_copied[3], ev_stage_a[3], ev_stage_b[3];
    hipEvent_t last_copied = nullptr;  // xfr_engine_wait_inputs_copied
    Event ev_slot_done[3];             // cross-step pipelining, with seedbuf[] below
    Event ev_tab;                      // the last host-to-device table copy (subtree scratch)
    std::unique_ptr<PhaseStreams> ph_streams;      // built at the first sweep through a strided KxK layer (backward.hip)
    std::vector<std::pair<Event, Event>> ev_pool;      // profiling: one pair per GEMM launch of a run
    // ---- buffers
    DevBuf<float> arena;               // parameters
    bool weights_loaded = false;
    DevBuf<float> fwd_ws[3];           // [0]: the whole workspace (forward slot 0, gradients, scratch); [1], [2]: the forward regions of pipeline slots 1 and 2
    DevBuf<float>& ws = fwd_ws[0];
    DevBuf<uint8_t> fwd_idx[3];        // max-pool argmax bytes, per forward slot
    DevBuf<double> dbl_ws;         // sums [2*maxB] + trace
    DevBuf<char> trunc_ws;
    DevBuf<float> ws_enc;          // second bank of true activations (T region only), allocated on first use
    DevBuf<uint8_t> u8_stage[3];         // the staging buffers of xfr_triplet_contrastive_u8_host: with their nine events one all-or-nothing group
    bool stage_busy[3] = {false, false, false};
    // the subtree scratch, one all-or-nothing group with ev_tab (ensure_subtree_scratch); cap_dev stands for it.  The tables of priors / captures are
    // staged in pinned host memory and copied once per call; the call's SweepCtx carries their device pointers to the sweep
    PinnedBuf<int> tab_elem_h;                        // prior element (or capture element) per (firing, row); -1: none
    DevBuf<int> tab_elem_d;
    PinnedBuf<float> tab_val_h;                       // prior value per (firing, row)
    DevBuf<float> tab_val_d;
    size_t tab_cap = 0;                               // entries allocated
    DevBuf<float> cap_dev;                            // [n_firings][rows] captured values
    DevBuf<float> stat_v;                             // [n_firings][max_batch]
    DevBuf<int> stat_i;
    DevBuf<char> stat_scratch;
    DevBuf<StatDesc> stat_desc;                       // [n_firings] tensor descriptors + firing -> tensor map of the last plan used
    DevBuf<int> stat_f2u;
    const void* stat_plan = nullptr;
    int stat_nu = 0;
    DevBuf<float> store_dev;                          // the full P tensor of one firing (xfr_ebp_store_firing)
    // xfr_weighted_subtree_ebp: row-max keys of a round (device + pinned host), the round's gather pairs and the merge table (device + pinned
    // host), and the top-k store used when the caller passes no top_dev (grown on demand)
    DevBuf<unsigned> wst_key_d;                       // the round buffers: one all-or-nothing group, wst_key_d stands for it
    PinnedBuf<unsigned> wst_key_h;
    DevBuf<int> wst_pairs_d, wst_cnt_d;
    PinnedBuf<int> wst_pairs_h, wst_cnt_h;
    DevBuf<SubtreeSlot> wst_tab_d;                    // the merge table: a pair of one capacity
    PinnedBuf<SubtreeSlot> wst_tab_h;
    DevBuf<float> wst_store;
    // tail-balancing scratch (conv_gemm.hip), one per stream that launches GEMMs; kernels on one stream serialise,
    // so consecutive launches share it
    struct TailWs { hipStream_t s; DevBuf<float> ws; unsigned* cnt; };
    TailWs tail_ws[8];
    int n_tail_ws = 0;
    std::unique_ptr<ProbeSweep> sweep;      // xfr_strise_* and xfr_inpaint_*: side stream, events, input and embedding buffers, built on first use
    std::unique_ptr<StriseState> strise;    // the families' own buffers, each built on its first call
    std::unique_ptr<InpaintState> inpaint;
    std::unique_ptr<MatchState> match;
    std::unique_ptr<IntakeState> intake;
    std::unique_ptr<FinishState> finish;
    // ---- options set through the ABI
    int mode = XFR_MODE_AFFINEONLY_WITH_PRIOR;
    float eps = 1e-16f;
    int with_bias = 0;
    int trace_on = 0;
    int profile_on = 0;
    std::string profile_csv;
    bool overlap_phases = true;        // the phases of one layer run side by side (they write disjoint pixels); profiled runs keep them in a row
    bool depthwise_valu = true;        // depthwise launches on the vector-ALU kernel (conv_depthwise.hip, configuration 14); fusion-mask bit 10 keeps them on 13
    bool tail_balance = true;          // xfr_engine_set_tail_balance
    bool split_forward = true;         // xfr_engine_set_forward_split: forward-only batches of >= 32 images as two halves on the internal streams
    bool interpret_chains = false;     // xfr_engine_set_epilogue_fusion bit 2: fused chains run through the interpreted epilogue (tests)
    bool planning_only = false;        // xfr_plan_describe: list what the planner WOULD fuse, whatever the signature table holds
    bool fuse_probe_fwd = true;        // probe forward (with the positive pass): BatchNorm / ReLU in the (dual) GEMM's epilogue (STORE raw, [FORK positive
                                       // BatchNorm], affine, clamp).  Round 3, MI355X: +0.6 % maps/s on ResNet-101, +2.2 % on ResNet-50-128d, bit-identical
    bool fuse_fwd_only = true;         // forward-only runs: BatchNorm / residual add / ReLU in the GEMM epilogue
    bool hoist_shortcut = true;        // down-sampling blocks: the shortcut (average pool, channel padding) is computed BEFORE the main path's last
                                       // convolution, so that the residual add joins its epilogue like in every other block (bit 8 of the fusion mask)
    bool direct_stem = true;           // Light-CNN's 1-channel 5x5 first layer as a direct convolution (xfr_engine_set_epilogue_fusion bit 4 clear; tests set it)
    bool fuse_avgup = true;            // down-sampling blocks: slice copy + pooled hook + average-pool VJP + strided GEMM's read-modify-write as the head of the
                                       // hook chain that follows (EW_AVGUP_IN; xfr_engine_set_epilogue_fusion bit 6 clear)
    bool fuse_branch = true;           // projection-shortcut blocks: the main path's hook chain as a side branch of the Add-output GEMM's epilogue (EW_STORE actions
                                       // 1 / 2; xfr_engine_set_epilogue_fusion bit 7 clear)
    bool pair_tiles = true;            // backward chain GEMMs over two streams walk their m-tiles stream-interleaved (xfr_engine_set_epilogue_fusion bit 5 clear)
    bool fuse_pools = true;            // Light-CNN's maxpool + avgpool pair: one forward kernel (xfr_engine_set_epilogue_fusion bit 0 switches it with the rest)
    bool fuse_gemm_epilogue = true;    // hook chains that follow a backward GEMM run in its (vector) epilogue
                                       // (both: xfr_engine_set_epilogue_fusion; DESIGN.md section 6 has the measurements)
    bool split_any_grid = false;       // xfr_engine_set_split_gemm mode + 4: covered layers take the bf16x6 kernel whatever the launch's grid (tests, tuning)
    int split_mask = 3;                // xfr_engine_set_split_gemm: which covered layers run the bf16x6 kernel (conv_gemm_split.hip K17) -- bit 0 the forward
                                       // convolutions, bit 1 the sweep's backward-data GEMMs; both by default since round 6 (short in-pipe sums)
    bool lean = true;                  // xfr_engine_set_lean: plain sweeps (no trace / prior / capture / stored firing, batch % 4 == 0) take the lean schedule
    // uint8 entry points (xfr_forward_u8 / xfr_triplet_contrastive_u8): the image pointer handed to the forward is uint8 H x W x C and the layout
    // kernel in front of the first convolution does the reference's preprocessing arithmetic (xfr_engine_set_u8_preprocess)
    bool u8_set = false;
    U8Pre u8_pre;
    bool u8_on = false;                // (Scoped) the running call is one of them
    bool inputs_ready = false;     // xfr_engine_set_inputs_ready: the NEXT level-2 call may read x_dev without waiting for the caller's stream (one-shot, ebp_core consumes it)
    // ---- profiling record: what the last traced / profiled run left for the getters
    int last_trace_firings = 0, last_trace_sb = 0;
    std::vector<int> last_trace_kinds;
    std::vector<ConvParams> ev_params;
    std::vector<int> ev_cfg;           // the configuration each profiled launch really ran
    double fam_ms[2] = {0.0, 0.0}, fam_flops[2] = {0.0, 0.0};      // last profiled run, by kernel family: [0] fp32 MFMA, [1] bf16x6
    long fam_launches[2] = {0, 0};
    size_t ev_used = 0;
    double prof_flops = 0.0;
    double last_gemm_ms = 0.0;
    long last_gemm_launches = 0;
    double last_gemm_flops = 0.0;
    // ---- pipeline slots: cross-step pipelining (xfr_engine_set_pipeline) -- two forward slots (T, Pv, norms, argmax) so that the forward of
    // triplet call i+1 may run while the backward sweep of call i still reads slot i%2
    bool pipeline = false;
    bool pipeline_all = false;     // level 2: xfr_ebp / xfr_contrastive calls are pipelined too ((Scoped) off around the image hook's sweep)
    int n_slots = 2;               // xfr_engine_set_pipeline bit 2: three forward slots (the forwards may run two calls ahead of the sweep)
    long seq = 0;
    DevBuf<float> seedbuf[3];
    bool slot_pending[3] = {false, false, false};
    int cur_slot = 0;              // (Scoped) the slot the running call's forward writes and its sweep reads; 0 between calls
    float* t_bank = nullptr;       // (Scoped) when set, true activations live in this bank (gallery forward of a triplet step)
    // ---- held forward.  xfr_engine_hold_forward: the forward state of (held_x, held_B, held_last) is still in slot 0
    bool hold_forward = false, held_pos = false;
    const float* held_x = nullptr;
    int held_B = 0, held_last = -1;
    hipStream_t held_stream = nullptr;
    std::vector<char> fwd_done;        // per forward pass: ops whose work was folded into an earlier GEMM epilogue
    std::vector<char> pos_done;        // ... and whose positive-pass output was produced there too
    int fwd_last_op = 0;
    // ---- lean run state
    const BwdPlan* lean_cur = nullptr; // (Scoped) the plan whose lean tables the running probe forward / sweep follow (null: literal)
    bool lean_decide = false;          // (Scoped) lean_prepare's dry run of the probe forward: decide per convolution, record in lean_q_run / lean_final_run
    bool dry_run = false;              // (Scoped) ... which launches nothing
    bool lean_missing_sig = false;     // ... and found a lean epilogue without a compiled signature
    long lean_launches = 0;            // dual-accumulator launches so far (xfr_engine_lean_stats)
    std::vector<char> lean_q_run;
    std::vector<int> lean_final_run;

    float* fwd_base() { return fwd_ws[cur_slot]; }
    uint8_t* idx_base() { return fwd_idx[cur_slot]; }
    float* T(int t) { const Tensor& x = tens[t]; return (t_bank ? t_bank : fwd_base()) + tens[x.alias >= 0 ? root(t) : t].t_off; }
    float* Pv(int t) { return fwd_base() + tens[t].pv_off; }
    float* misc() { return fwd_base() + misc_off; }
    float* G(int t) { return ws + tens[t].g_off; }
    int root(int t) const { while (tens[t].alias >= 0) t = tens[t].alias; return t; }
    size_t max_per_n() const { size_t m = 0; for (const Tensor& x : tens) m = std::max(m, (size_t)x.per_n()); return m; }      // elements per sample of the largest tensor
};

// xfr_weighted_subtree_ebp holds one forward for all its phases: the caller's hold (an enclosing group) survives the call, ours ends with it -- and
// drops the held forward, which a plain Scoped<bool> would not
struct HoldGuard {
    xfr_engine* e;
    const bool prev;
    explicit HoldGuard(xfr_engine* e_) : e(e_), prev(e_->hold_forward) { if (!prev) { e->hold_forward = true; e->held_x = nullptr; } }
    ~HoldGuard() { if (!prev) { e->hold_forward = false; e->held_x = nullptr; } }
    HoldGuard(const HoldGuard&) = delete;
    HoldGuard& operator=(const HoldGuard&) = delete;
};

namespace xfr {

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline bool is_affine_name(int kind)
{   // whitebox.py:399/:409: 'Conv' | 'Linear' | 'AvgPool' | 'BatchNorm' in str(module)
    return kind == XFR_OP_CONV || kind == XFR_OP_LINEAR || kind == XFR_OP_AVGPOOL || kind == XFR_OP_BATCHNORM;
}

// plan.hip (device-free)
xfr_status build(xfr_engine* e, const xfr_op_desc* ops, int n_ops);
void compute_need(xfr_engine* e);
xfr_status layout_workspace(xfr_engine* e);
xfr_status layout_arena(xfr_engine* e);
xfr_status get_plan(xfr_engine* e, int seed_tensor, BwdPlan** out, bool plain = false);

// plan_fuse.hip (device-free)
void fuse_plan(xfr_engine* e, BwdPlan& plan);
void lean_rewrite_plan(xfr_engine* e, BwdPlan& plan);

// forward.hip
xfr_status run_conv(xfr_engine* e, const ConvParams& p_in, hipStream_t s);
void conv_geometry(xfr_engine* e, int k, int NB, ConvParams& p);
void fuse_forward_only(xfr_engine* e, int k, int B, ConvParams& p, hipStream_t s);
void fuse_probe_forward(xfr_engine* e, int k, int B, ConvParams& p, hipStream_t s, bool dual = false, bool lean_try = true);
bool fuse_mfm_forward(xfr_engine* e, int k, int B, bool keep_raw, ConvParams& p, bool want_pos = true);
// keep_raw: no positive pass, but a plain-weight backward pass follows (xfr_subtree_weights): the MaxFeatureMap forwards still store the raw halves its VJP reads
xfr_status forward_all(xfr_engine* e, const float* x_dev, int B, int last_tensor, bool with_pos, hipStream_t s, bool keep_raw = false);
void lean_prepare(xfr_engine* e, BwdPlan& plan, int B);
bool lean_applies(xfr_engine* e, BwdPlan& plan, int B, const SweepCtx& cx);

// backward.hip
void resolve_chain(xfr_engine* e, const SweepCtx& cx, const std::vector<BwdStep::Sym>& syms, EwChain& ch, double* trace, int SB, bool plain = false);
xfr_status run_backward(xfr_engine* e, const SweepCtx& cx, BwdPlan& plan, int B, int S, hipStream_t s);
bool bwd_conv_params(xfr_engine* e, const SweepCtx& cx, const BwdPlan& plan, const BwdStep& st, int B, int SB, int SBa, ConvParams& p, const PhaseRec* ph = nullptr);

// engine.hip
xfr_status check_run(xfr_engine* e, const void* x, int n);
xfr_status fence_slot0(xfr_engine* e, hipStream_t s);
xfr_status ebp_core(xfr_engine* e, const SweepCtx& cx, const float* x_dev, int n, int S, int seed_tensor, const float* seed_dev, hipStream_t s);
xfr_status require_u8(xfr_engine* e);                                       // precondition of every uint8 entry point

// weights.hip
// row of (input channel ci, tap tp) in a forward pack: (kh,kw,4 channel slots) for image stems, tap-major (kh,kw,ci), or (ci,kh,kw)
inline size_t forward_pack_row(bool tap4, bool tap, int ci, int tp, int cin, int khw)
{
    return tap4 ? (size_t)tp * 4 + ci : (tap ? (size_t)tp * cin + ci : (size_t)ci * khw + tp);
}
xfr_status pack_weights(const xfr_engine* e, const xfr_tensor_view* w, std::vector<float>& host);       // every pack of the arena, on the host
void presplit_weights(xfr_engine* e);

// probe_sweep.hip.  Every xfr_strise_* / xfr_inpaint_* entry point that touches device state runs between sweep_enter, after its argument checks,
// and sweep_leave (SweepCall does the latter on every way out), so calls on one engine are ordered one behind another whatever their streams.
xfr_status sweep_enter(xfr_engine* e, hipStream_t s, ProbeSweep** sw);      // hipSetDevice; `s` waits for the side stream's tail and the previous call's end
void sweep_leave(ProbeSweep* sw, hipStream_t s);                            // records the end of this call on `s`
struct SweepCall {
    ProbeSweep* sw = nullptr;
    hipStream_t s = nullptr;
    xfr_status enter(xfr_engine* e, hipStream_t stream) { s = stream; return sweep_enter(e, s, &sw); }
    ~SweepCall() { if (sw) sweep_leave(sw, s); }
};
xfr_status sweep_side_follows(ProbeSweep* sw, hipStream_t s);               // the side stream waits for what `s` holds now
// the batch loop over ceil(n_images / max_batch) batches: generate(i, xbuf, side stream) launches the max_batch images of batch i (padding included),
// consume(i, emb, s) what reads their embeddings; the buffer hand-over, xfr_forward and the join of the side stream on an error are the loop's
using SweepGenerate = std::function<void(long, float*, hipStream_t)>;
using SweepConsume = std::function<void(long, const float*, hipStream_t)>;
xfr_status run_sweep(xfr_engine* e, ProbeSweep* sw, long n_images, int encode_tensor, hipStream_t s, const SweepGenerate& generate,
                     const SweepConsume& consume);

// strise_abi.hip
xfr_status check_taps(const xfr_strise_tap* tab, int entries, int n, const char* what, const char* who);

}  // namespace xfr
