// engine.hip -- the C ABI (include/xfr_amd.h) of the EBP engine: engine life cycle, weights, switches, the forward / EBP / contrastive / triplet
// entry points with their stream choreography, the uint8 inputs and the profiling getters.  The planner is plan.hip + plan_fuse.hip, the executors
// forward.hip + backward.hip; the packs of the weight arena are weights.hip's; the layerwise / weighted-subtree entry points are in subtree.hip, the
// xfr_debug_* ones in debug_abi.hip, RCCL in comm.hip, xfr_plan_describe in plan_describe.hip.
#include "engine_internal.h"

namespace xfr {

static xfr_status allocate(xfr_engine* e)
{
    xfr_status st = layout_arena(e);
    if (st != XFR_OK) return st;
    XFR_TRY(e->arena.alloc(e->arena_floats));
    st = layout_workspace(e);
    if (st != XFR_OK) return st;
    const size_t B = (size_t)e->max_batch;
    XFR_TRY(e->ws.alloc(e->ws_floats));
    XFR_TRY(e->fwd_idx[0].alloc(e->idx_bytes));
    size_t hooks = 0;
    for (auto& x : e->tens) hooks += x.hooks.size();
    e->trace_cap = hooks;
    XFR_TRY(e->dbl_ws.alloc(2 * B + hooks * 2 * B + 64));
    XFR_TRY(e->trunc_ws.alloc(truncation_scratch_bytes((int)B)));
    return XFR_OK;
}

xfr_status check_run(xfr_engine* e, const void* x, int n)
{
    if (!e) return fail(XFR_INVALID_ARG, "null engine");
    if (!e->weights_loaded) return fail(XFR_STATE_ERROR, "weights not loaded");
    if (!x) return fail(XFR_INVALID_ARG, "null input");
    if (n < 1 || n > e->max_batch) return fail(XFR_INVALID_ARG, "batch %d outside [1, %d]", n, e->max_batch);
    HIP_TRY(hipSetDevice(e->device));
    if (e->need_dirty) compute_need(e);
    return XFR_OK;
}

static void prof_begin(xfr_engine* e) { e->ev_used = 0; e->prof_flops = 0.0; }

static xfr_status prof_end(xfr_engine* e, hipStream_t s)
{
    if (!e->profile_on) return XFR_OK;
    HIP_TRY(hipStreamSynchronize(s));
    double ms = 0.0;
    FILE* f = e->profile_csv.empty() ? nullptr : fopen(e->profile_csv.c_str(), "a");   // per-launch GEMM records (xfr_engine_profile_csv)
    for (int q = 0; q < 2; ++q) { e->fam_ms[q] = 0.0; e->fam_flops[q] = 0.0; e->fam_launches[q] = 0; }
    for (size_t i = 0; i < e->ev_used; ++i) {
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, e->ev_pool[i].first, e->ev_pool[i].second));
        ms += t;
        const ConvParams& p = e->ev_params[i];
        const int Kl = p.K_logical ? p.K_logical : p.K;
        const double fl = 2.0 * Kl * (double)p.M * p.CoutTot * (p.dualacc ? 2 : p.nhalves);
        const int fam = e->ev_cfg[i] == CFG_BF16X6 ? 1 : 0;
        e->fam_ms[fam] += t; e->fam_flops[fam] += fl; e->fam_launches[fam] += 1;
        if (f) fprintf(f, "%d,%d,%d,%d,%d,%d,%d,%d,%d,%.4f,%.2f,%d\n", p.CoutTot, p.nhalves, Kl, p.M, p.kh, p.stride, p.out_stride,
                       p.relu_in, p.accumulate, t, fl / (t * 1e-3) / 1e12, e->ev_cfg[i]);
    }
    if (f) fclose(f);
    e->last_gemm_ms = ms;
    e->last_gemm_launches = (long)e->ev_used;
    e->last_gemm_flops = e->prof_flops;
    return XFR_OK;
}

// The fork of the internal streams: `a` (and `b`, when given) start behind everything already on the caller's stream `s` ...
static xfr_status fork_streams(xfr_engine* e, hipStream_t s, hipStream_t a, hipStream_t b = nullptr)
{
    HIP_TRY(hipEventRecord(e->ev_fork, s));
    HIP_TRY(hipStreamWaitEvent(a, e->ev_fork, 0));
    if (b) HIP_TRY(hipStreamWaitEvent(b, e->ev_fork, 0));
    return XFR_OK;
}

// ... and the join: `s` goes on behind what `a` (when given) and `b` hold now
static xfr_status join_streams(xfr_engine* e, hipStream_t s, hipStream_t a, hipStream_t b)
{
    if (a) HIP_TRY(hipEventRecord(e->ev_a, a));
    HIP_TRY(hipEventRecord(e->ev_b, b));
    if (a) HIP_TRY(hipStreamWaitEvent(s, e->ev_a, 0));
    HIP_TRY(hipStreamWaitEvent(s, e->ev_b, 0));
    return XFR_OK;
}

// Any run that used forward slot 0 outside the pipelined paths must fence it, or a later pipelined forward (internal
// stream) could overwrite activations this run's kernels on `s` are still using.
xfr_status fence_slot0(xfr_engine* e, hipStream_t s)
{
    if (e->pipeline && e->ev_slot_done[0]) {
        HIP_TRY(hipEventRecord(e->ev_slot_done[0], s));
        e->slot_pending[0] = true;
    }
    return XFR_OK;
}

xfr_status ebp_core(xfr_engine* e, const SweepCtx& cx, const float* x_dev, int n, int S, int seed_tensor, const float* seed_dev, hipStream_t s)
{
    // the one-shot promise of xfr_engine_set_inputs_ready covers THIS call, whatever becomes of it: consumed before the first check that
    // can fail, so an early error never leaves it standing for a later call that declared nothing
    const bool ready = e->inputs_ready;
    e->inputs_ready = false;
    if (seed_tensor < 2 || seed_tensor >= (int)e->tens.size()) return fail(XFR_INVALID_ARG, "bad seed tensor %d", seed_tensor);
    if (!seed_dev) return fail(XFR_INVALID_ARG, "null seed");
    BwdPlan* plan = nullptr;
    xfr_status st = get_plan(e, seed_tensor, &plan);
    if (st != XFR_OK) return st;
    // pipeline level 2: the forward of this call runs on an internal stream and only waits for the slot it overwrites, so it
    // overlaps the backward sweep of the previous call (which is still reading the other slot)
    const bool pipe = e->pipeline_all && !e->profile_on && e->s_b;
    hipStream_t sf = pipe ? e->s_b : s;
    const int slot = pipe ? (int)(e->seq++ % e->n_slots) : 0;
    Scoped<int> cur_slot(e->cur_slot, slot);
    if (pipe && e->slot_pending[slot]) HIP_TRY(hipStreamWaitEvent(sf, e->ev_slot_done[slot], 0));
    // (the promise covers ONE call: a caller that forgets to renew it falls back to the safe ordering, never to a stale promise)
    if (pipe && !ready) {
        // x_dev may still be pending on the caller's stream (a cast, a copy): order the internal forward after it.  Callers
        // whose inputs are resident declare it with xfr_engine_set_inputs_ready and keep the cross-call overlap.
        XFR_TRY(fork_streams(e, s, sf));
    }
    Scoped<const BwdPlan*> lean_cur(e->lean_cur, lean_applies(e, *plan, n, cx) ? plan : nullptr);
    st = forward_all(e, x_dev, n, seed_tensor, true, sf);
    if (st != XFR_OK) return st;
    if (pipe) XFR_TRY(join_streams(e, s, nullptr, sf));
    const Tensor& sd = e->tens[seed_tensor];
    launch_seed_to_cnhw(seed_dev, e->G(seed_tensor), S * n, sd.C, sd.HW(), s);
    st = run_backward(e, cx, *plan, n, S, s);
    if (pipe && st == XFR_OK) {
        HIP_TRY(hipEventRecord(e->ev_slot_done[slot], s));
        e->slot_pending[slot] = true;
    } else if (st == XFR_OK) {
        st = fence_slot0(e, s);
    }
    return st;
}

// precondition of every uint8 entry point
xfr_status require_u8(xfr_engine* e)
{
    if (!e) return fail(XFR_INVALID_ARG, "null engine");
    if (!e->u8_set) return fail(XFR_STATE_ERROR, "xfr_engine_set_u8_preprocess has not been called");
    return XFR_OK;
}

}  // namespace xfr

// ===================================================================================================================
extern "C" {

int32_t xfr_abi_version(void) { return XFR_AMD_ABI_VERSION; }

const char* xfr_last_error(void) { return g_err.c_str(); }

xfr_status xfr_engine_create(const xfr_op_desc* ops, int32_t n_ops, int32_t n_weights, int32_t in_c, int32_t in_h, int32_t in_w,
                             int32_t max_batch, int32_t device, xfr_engine** out)
{
    if (!ops || n_ops < 2 || !out || in_c < 1 || in_h < 1 || in_w < 1 || max_batch < 1 || n_weights < 0)
        return fail(XFR_INVALID_ARG, "xfr_engine_create: bad arguments");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(XFR_HIP_ERROR, "no HIP device visible: the xfr_amd engine has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(XFR_INVALID_ARG, "device %d out of range (%d visible)", device, ndev);
    HIP_TRY(hipSetDevice(device));
    if (ops[0].kind != XFR_OP_CONV || ops[0].in0 != 0)
        return fail(XFR_UNSUPPORTED_LAYER, "the first layer must be a convolution on the input image");
    xfr_engine* e = new xfr_engine();
    e->device = device; e->max_batch = max_batch; e->in_c = in_c; e->in_h = in_h; e->in_w = in_w; e->n_weights = n_weights;
    xfr_status st = build(e, ops, n_ops);
    if (st == XFR_OK) st = allocate(e);
    if (st != XFR_OK) { xfr_engine_destroy(e); return st; }
    if (const char* v = getenv("XFR_SPLIT_GEMM")) { e->split_mask = atoi(v) & 3; e->split_any_grid = (atoi(v) & 4) != 0; }      // A/B runs: the mode of xfr_engine_set_split_gemm for new engines
    *out = e;
    return XFR_OK;
}

xfr_status xfr_engine_destroy(xfr_engine* e)
{
    if (!e) return XFR_OK;
    (void)hipSetDevice(e->device);
    if (e->arena) conv_gemm_forget_split(e->arena, e->arena_floats * sizeof(float));      // before the arena goes: its bf16 planes (K17)
    delete e;
    return XFR_OK;
}

xfr_status xfr_engine_load_weights(xfr_engine* e, const xfr_tensor_view* w, int32_t n_weights)
{
    if (e) e->held_x = nullptr;
    if (!e || !w) return fail(XFR_INVALID_ARG, "null argument");
    if (n_weights != e->n_weights) return fail(XFR_INVALID_ARG, "expected %d weight views, got %d", e->n_weights, n_weights);
    HIP_TRY(hipSetDevice(e->device));
    std::vector<float> host;
    const xfr_status st = pack_weights(e, w, host);
    if (st != XFR_OK) return st;
    conv_gemm_forget_split(e->arena, e->arena_floats * sizeof(float));          // bf16 planes of the old weights (K17)
    HIP_TRY(hipMemcpy(e->arena, host.data(), e->arena_floats * sizeof(float), hipMemcpyHostToDevice));
    e->weights_loaded = true;
    presplit_weights(e);
    return XFR_OK;
}

xfr_status xfr_engine_weight_arena(xfr_engine* e, void** dev_ptr, size_t* bytes)
{
    if (!e || !dev_ptr || !bytes) return fail(XFR_INVALID_ARG, "null argument");
    *dev_ptr = e->arena;              // (a caller that writes through it ends with xfr_engine_mark_weights_loaded, which rebuilds the bf16 planes of K17)
    *bytes = e->arena_floats * sizeof(float);
    return XFR_OK;
}

xfr_status xfr_engine_mark_weights_loaded(xfr_engine* e)
{
    if (e) e->held_x = nullptr;
    if (!e) return fail(XFR_INVALID_ARG, "null engine");
    e->weights_loaded = true;
    // the caller wrote the arena (through a pointer it may have held across forwards): planes built from the old contents are stale
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    conv_gemm_forget_split(e->arena, e->arena_floats * sizeof(float));
    presplit_weights(e);
    return XFR_OK;
}

xfr_status xfr_engine_set_mode(xfr_engine* e, int32_t subtree_mode, float eps, int32_t with_bias)
{
    if (!e) return fail(XFR_INVALID_ARG, "null engine");
    if (subtree_mode < 0 || subtree_mode > 3) return fail(XFR_INVALID_ARG, "Invalid subtree mode %d", subtree_mode);
    if (!(eps >= 0.f)) return fail(XFR_INVALID_ARG, "eps must be >= 0");
    const int wb = with_bias ? 1 : 0;
    if (e->mode == subtree_mode && e->eps == eps && e->with_bias == wb) return XFR_OK;     // nothing to re-plan
    e->mode = subtree_mode; e->eps = eps; e->with_bias = wb;
    e->need_dirty = true;
    e->held_x = nullptr;
    return XFR_OK;
}

xfr_status xfr_engine_tensor_shape(xfr_engine* e, int32_t t, int32_t* c, int32_t* h, int32_t* w)
{
    if (!e || t < 0 || t >= (int)e->tens.size()) return fail(XFR_INVALID_ARG, "bad tensor id");
    if (c) *c = e->tens[t].C;
    if (h) *h = e->tens[t].H;
    if (w) *w = e->tens[t].W;
    return XFR_OK;
}

static xfr_status ensure_streams(xfr_engine* e);

xfr_status xfr_forward(xfr_engine* e, const float* x_dev, int32_t n, int32_t tensor_id, float* out_dev, void* stream)
{
    xfr_status st = check_run(e, x_dev, n);
    if (st != XFR_OK) return st;
    if (tensor_id < 1 || tensor_id >= (int)e->tens.size() || !out_dev) return fail(XFR_INVALID_ARG, "bad tensor id / null output");
    hipStream_t s = (hipStream_t)stream;
    prof_begin(e);
    // A forward-only batch (whitebox.py:747-785 embeddings; blackbox.py:366-414 scores ~6500 masked copies of a probe with it) as two half
    // batches on the two internal streams, like the gallery / probe pair of a triplet step: a layer's launches of the two halves fill each
    // other's prologues, epilogues and tails (round 3: one stream reached 0.52 of the fp32 MFMA peak).  The first half runs in the second
    // activation region (the one the triplet step's gallery forward uses); images are independent, the halves meet on the caller's stream.
    const int n0 = (n / 2) & ~3;
    if (e->split_forward && !e->profile_on && !e->hold_forward && n >= 32 && n0 >= 8) {
        if (!e->ws_enc) XFR_TRY(e->ws_enc.alloc(e->t_region_floats + 4096));
        st = ensure_streams(e);
        if (st != XFR_OK) return st;
        const Tensor& t = e->tens[tensor_id];
        const size_t in_per_n = (size_t)e->in_c * e->in_h * e->in_w;
        XFR_TRY(fork_streams(e, s, e->s_a, e->s_b));      // after everything already on the caller's stream (inputs, earlier sweeps)
        // whatever was enqueued on the internal streams (also by a half that then failed) is ordered before anything the caller puts on s next
        auto join = [&]() -> xfr_status { return join_streams(e, s, e->s_a, e->s_b); };
        {
            Scoped<float*> bank(e->t_bank, e->ws_enc);
            st = forward_all(e, x_dev, n0, tensor_id, false, e->s_a);
            if (st != XFR_OK) { const std::string why = g_err; join(); g_err = why; return st; }
            launch_cnhw_to_nchw(e->T(tensor_id), out_dev, n0, t.C, t.HW(), e->s_a);
        }
        const float* x_hi = e->u8_on ? reinterpret_cast<const float*>(reinterpret_cast<const uint8_t*>(x_dev) + (size_t)n0 * e->in_h * e->in_w * e->u8_pre.channels)
                                     : x_dev + (size_t)n0 * in_per_n;
        st = forward_all(e, x_hi, n - n0, tensor_id, false, e->s_b);
        if (st != XFR_OK) { const std::string why = g_err; join(); g_err = why; return st; }
        launch_cnhw_to_nchw(e->T(tensor_id), out_dev + (size_t)n0 * t.per_n(), n - n0, t.C, t.HW(), e->s_b);
        st = join();
        if (st != XFR_OK) return st;
        HIP_TRY(hipGetLastError());
        st = fence_slot0(e, s);
        if (st != XFR_OK) return st;
        return prof_end(e, s);
    }
    st = forward_all(e, x_dev, n, tensor_id, false, s);
    if (st != XFR_OK) return st;
    const Tensor& t = e->tens[tensor_id];
    launch_cnhw_to_nchw(e->T(tensor_id), out_dev, n, t.C, t.HW(), s);
    HIP_TRY(hipGetLastError());
    st = fence_slot0(e, s);
    if (st != XFR_OK) return st;
    return prof_end(e, s);
}

xfr_status xfr_ebp(xfr_engine* e, const float* x_dev, int32_t n, int32_t n_streams, int32_t seed_tensor, const float* seed_dev,
                   float* mwp_dev, float* pooled_dev, void* stream)
{
    xfr_status st = check_run(e, x_dev, n);
    if (st != XFR_OK) return st;
    if (n_streams < 1 || n_streams > 2) return fail(XFR_INVALID_ARG, "n_streams must be 1 or 2");
    hipStream_t s = (hipStream_t)stream;
    prof_begin(e);
    st = ebp_core(e, SweepCtx(), x_dev, n, n_streams, seed_tensor, seed_dev, s);
    if (st != XFR_OK) return st;
    const Tensor& t1 = e->tens[1];
    const int SB = n_streams * n;
    if (mwp_dev) launch_cnhw_to_nchw(e->ws + e->tap_off, mwp_dev, SB, t1.C, t1.HW(), s);
    if (pooled_dev) launch_channel_pool(e->ws + e->tap_off, pooled_dev, t1.C, SB, t1.HW(), s);
    HIP_TRY(hipGetLastError());
    return prof_end(e, s);
}

static xfr_status ensure_streams(xfr_engine* e)
{
    if (e->s_a) return XFR_OK;
    // The internal streams run forwards -- in pipelined mode the NEXT call's -- while the caller's stream runs the backward
    // sweep whose maps the caller waits for: the forwards take the lowest priority, so the dispatcher prefers the sweep's
    // workgroups when both have some ready (measured on MI355X: 26.81 -> 26.69 ms per step; forwards at high priority: 27.3)
    int lowest = 0, highest = 0;
    HIP_TRY(hipDeviceGetStreamPriorityRange(&lowest, &highest));
    Stream a, b;
    Event fork, ev_a, ev_b;
    XFR_TRY(a.create(lowest));
    XFR_TRY(b.create(lowest));
    XFR_TRY(fork.create());
    XFR_TRY(ev_a.create());
    XFR_TRY(ev_b.create());
    e->s_a = std::move(a); e->s_b = std::move(b);
    e->ev_fork = std::move(fork); e->ev_a = std::move(ev_a); e->ev_b = std::move(ev_b);
    return XFR_OK;
}

enum ContrastTail { TAIL_V6 = 0, TAIL_RAW = 1, TAIL_U8 = 2 };      // _mwp_to_saliency of ebp_version 6 (float maps) / none / of the other versions (bytes)

static xfr_status contrastive_tail(xfr_engine* e, int n, float percentile, void* out_dev, hipStream_t s, ContrastTail tail = TAIL_V6)
{
    const Tensor& t1 = e->tens[1];
    const float* P = e->ws + e->tap_off;
    double* sums = e->dbl_ws;
    launch_sample_sums(P, sums, t1.C, 2 * n, t1.HW(), s);
    float* thr = nullptr;
    if (percentile >= 0.f) {
        thr = e->ws + e->thr_off;
        launch_truncation_threshold(P, sums, percentile, thr, e->trunc_ws, t1.C, n, t1.HW(), s);
    }
    float* contrast = tail == TAIL_RAW ? static_cast<float*>(out_dev) : e->ws + e->blur_a_off;
    launch_contrast(P, sums, thr, contrast, t1.C, n, t1.HW(), s);
    if (tail == TAIL_V6) launch_saliency_blur(contrast, e->ws + e->blur_b_off, static_cast<float*>(out_dev), n, t1.H, t1.W, e->eps, s);
    if (tail == TAIL_U8) launch_u8_tail(contrast, nullptr, false, static_cast<unsigned char*>(out_dev), nullptr, n, t1.H, t1.W, e->eps, s);
    HIP_TRY(hipGetLastError());
    return XFR_OK;
}

// the uint8 tail keeps a whole map in one workgroup's LDS
static xfr_status check_u8_tail(xfr_engine* e, const char* who)
{
    const Tensor& t1 = e->tens[1];
    if ((long)t1.H * t1.W > U8_TAIL_MAX_HW)
        return fail(XFR_INVALID_ARG, "%s: maps of %d x %d exceed the %d pixels of the uint8 tail", who, t1.H, t1.W, U8_TAIL_MAX_HW);
    return XFR_OK;
}

// xfr_contrastive / xfr_contrastive_raw / xfr_contrastive_u8: raw = the truncated contrast itself, without the saliency blur
static xfr_status contrastive(xfr_engine* e, const float* x_dev, int32_t n, int32_t seed_tensor, const float* seed_dev, float percentile,
                              void* out_dev, void* stream, ContrastTail tail)
{
    xfr_status st = check_run(e, x_dev, n);
    if (st != XFR_OK) return st;
    if (!out_dev) return fail(XFR_INVALID_ARG, "null output");
    if (tail == TAIL_U8) {
        st = check_u8_tail(e, "xfr_contrastive_u8");
        if (st != XFR_OK) return st;
    }
    if (percentile > 100.f) return fail(XFR_INVALID_ARG, "percentile must be <= 100 (or < 0 for plain contrastive)");
    hipStream_t s = (hipStream_t)stream;
    prof_begin(e);
    st = ebp_core(e, SweepCtx(), x_dev, n, 2, seed_tensor, seed_dev, s);
    if (st != XFR_OK) return st;
    st = contrastive_tail(e, n, percentile, out_dev, s, tail);
    if (st != XFR_OK) return st;
    return prof_end(e, s);
}

xfr_status xfr_contrastive(xfr_engine* e, const float* x_dev, int32_t n, int32_t seed_tensor, const float* seed_dev,
                           float percentile, float* sal_dev, void* stream)
{
    return contrastive(e, x_dev, n, seed_tensor, seed_dev, percentile, sal_dev, stream, TAIL_V6);
}

xfr_status xfr_contrastive_raw(xfr_engine* e, const float* x_dev, int32_t n, int32_t seed_tensor, const float* seed_dev,
                               float percentile, float* contrast_dev, void* stream)
{
    return contrastive(e, x_dev, n, seed_tensor, seed_dev, percentile, contrast_dev, stream, TAIL_RAW);
}

xfr_status xfr_contrastive_u8(xfr_engine* e, const float* x_dev, int32_t n, int32_t seed_tensor, const float* seed_dev,
                              float percentile, uint8_t* sal_dev, void* stream)
{
    return contrastive(e, x_dev, n, seed_tensor, seed_dev, percentile, sal_dev, stream, TAIL_U8);
}

// xfr_triplet_contrastive (float maps, the ebp_version 6 tail) and xfr_triplet_contrastive_u8tail (bytes, the tail of the other versions).
// in_ev / stage_slot, the engine's own staging (xfr_triplet_contrastive_u8_host; nullptr / -1 otherwise): the inputs are complete when the copy's event
// fires -- nothing on the caller's stream concerns them, so the forwards of a pipelined call need not wait for it -- and sit in that staging slot
static xfr_status triplet_contrastive(xfr_engine* e, const float* probes_dev, const float* gallery_dev, int32_t n,
                                      int32_t encode_tensor, float scale, float percentile, void* sal_dev, void* stream,
                                      int32_t inputs_ready, ContrastTail tail, hipEvent_t in_ev, int stage_slot)
{
    xfr_status st = check_run(e, probes_dev, n);
    if (st != XFR_OK) return st;
    if (!gallery_dev || !sal_dev) return fail(XFR_INVALID_ARG, "null argument");
    if (tail == TAIL_U8) {
        st = check_u8_tail(e, "xfr_triplet_contrastive_u8tail");
        if (st != XFR_OK) return st;
    }
    if (2 * n > e->max_batch) return fail(XFR_INVALID_ARG, "triplet batch %d needs max_batch >= %d (the gallery forward runs 2n images)", n, 2 * n);
    if (percentile > 100.f) return fail(XFR_INVALID_ARG, "percentile must be <= 100 (or < 0 for plain contrastive)");
    if (encode_tensor < 2 || encode_tensor >= (int)e->tens.size()) return fail(XFR_INVALID_ARG, "bad encode tensor %d", encode_tensor);
    hipStream_t s = (hipStream_t)stream;
    if (!e->ws_enc) XFR_TRY(e->ws_enc.alloc(e->t_region_floats + 4096));
    {
        xfr_status es = ensure_streams(e);
        if (es != XFR_OK) return es;
    }
    BwdPlan* plan = nullptr;
    st = get_plan(e, encode_tensor, &plan);
    if (st != XFR_OK) return st;
    prof_begin(e);
    // The gallery encodes (2n images, true weights only) and the probe forward (n images, W and relu(W)) are
    // independent until the backward sweep needs its seeds: run them on two streams so their small layer-3/4 grids
    // fill each other's idle CUs.  With profiling on, everything is serialised on the caller's stream instead.
    // In pipeline mode the forwards do not wait for the caller's stream at all (only for the slot they overwrite), so
    // the forward of call i+1 overlaps the backward sweep of call i.
    const bool fork = !e->profile_on;
    const bool pipe = fork && e->pipeline;
    hipStream_t sa = fork ? e->s_a : s, sb = fork ? e->s_b : s;
    // every exit path (errors included) leaves the engine on slot 0 / the main bank: the non-pipelined entry points assume it
    const int slot = pipe ? (int)(e->seq++ % e->n_slots) : 0;
    Scoped<int> cur_slot(e->cur_slot, slot);
    if (fork) {
        if (pipe && (inputs_ready || in_ev)) {
            if (e->slot_pending[slot]) {       // the backward that last read this slot must be done
                HIP_TRY(hipStreamWaitEvent(sa, e->ev_slot_done[slot], 0));
                HIP_TRY(hipStreamWaitEvent(sb, e->ev_slot_done[slot], 0));
            }
        } else {                               // order the forwards after everything already on the caller's stream
            XFR_TRY(fork_streams(e, s, sa, sb));
        }
        if (in_ev) {
            HIP_TRY(hipStreamWaitEvent(sa, in_ev, 0));
            HIP_TRY(hipStreamWaitEvent(sb, in_ev, 0));
        }
    } else if (in_ev) HIP_TRY(hipStreamWaitEvent(s, in_ev, 0));
    const Tensor& sd = e->tens[encode_tensor];
    float* seed_dst = pipe ? e->seedbuf[slot] : e->G(encode_tensor);
    {
        Scoped<float*> bank(e->t_bank, e->ws_enc);
        st = forward_all(e, gallery_dev, 2 * n, encode_tensor, false, sa);
        // seeds: stream 0 = scale * encode(mate_i), stream 1 = scale * encode(nonmate_i)  (demo/test_whitebox.py:129 with the
        // one-hot priors of whitebox.py:512,518 folded through the un-hooked 2-way classifier).  Layouts coincide:
        // both are [D][2n][1].
        if (st == XFR_OK) launch_scale(e->T(encode_tensor), seed_dst, (long)sd.per_n() * 2 * n, scale, 0, sa);
    }
    if (st != XFR_OK) return st;
    const SweepCtx plain;
    Scoped<const BwdPlan*> lean_cur(e->lean_cur, lean_applies(e, *plan, n, plain) ? plan : nullptr);
    st = forward_all(e, probes_dev, n, encode_tensor, true, sb);
    if (st != XFR_OK) return st;
    if (fork) XFR_TRY(join_streams(e, s, sa, sb));
    if (stage_slot >= 0) {                     // the staging buffer may be overwritten once both forwards have read it
        HIP_TRY(hipEventRecord(e->ev_stage_a[stage_slot], sa));
        HIP_TRY(hipEventRecord(e->ev_stage_b[stage_slot], sb));
        e->stage_busy[stage_slot] = true;
    }
    if (pipe) launch_copy_acc(seed_dst, e->G(encode_tensor), (long)sd.per_n() * 2 * n, 0, s);
    st = run_backward(e, plain, *plan, n, 2, s);
    if (st != XFR_OK) return st;
    st = contrastive_tail(e, n, percentile, sal_dev, s, tail);
    if (st != XFR_OK) return st;
    if (pipe) {
        HIP_TRY(hipEventRecord(e->ev_slot_done[slot], s));
        e->slot_pending[slot] = true;
    }
    return prof_end(e, s);
}

xfr_status xfr_triplet_contrastive(xfr_engine* e, const float* probes_dev, const float* gallery_dev, int32_t n,
                                   int32_t encode_tensor, float scale, float percentile, float* sal_dev, void* stream,
                                   int32_t inputs_ready)
{
    return triplet_contrastive(e, probes_dev, gallery_dev, n, encode_tensor, scale, percentile, sal_dev, stream, inputs_ready, TAIL_V6, nullptr, -1);
}

xfr_status xfr_triplet_contrastive_u8tail(xfr_engine* e, const float* probes_dev, const float* gallery_dev, int32_t n,
                                          int32_t encode_tensor, float scale, float percentile, uint8_t* sal_dev, void* stream,
                                          int32_t inputs_ready)
{
    return triplet_contrastive(e, probes_dev, gallery_dev, n, encode_tensor, scale, percentile, sal_dev, stream, inputs_ready, TAIL_U8, nullptr, -1);
}

xfr_status xfr_engine_set_u8_preprocess(xfr_engine* e, const xfr_u8_preprocess* p)
{
    if (!e || !p) return fail(XFR_INVALID_ARG, "null argument");
    if (p->kind == XFR_U8_SUB_MEAN) {
        if (p->channels != e->in_c || p->channels > 4) return fail(XFR_INVALID_ARG, "uint8 preprocessing: %d image channels for a %d-channel network input", p->channels, e->in_c);
    } else if (p->kind == XFR_U8_LUMINANCE) {
        if (p->channels != 3 || e->in_c != 1) return fail(XFR_INVALID_ARG, "uint8 luminance preprocessing takes 3-channel images into a 1-channel network input");
    } else return fail(XFR_INVALID_ARG, "unknown uint8 preprocessing kind %d", p->kind);
    e->u8_pre.kind = p->kind;
    e->u8_pre.channels = p->channels;
    for (int i = 0; i < 4; ++i) { e->u8_pre.mean[i] = p->mean[i]; e->u8_pre.weight[i] = p->weight[i]; }
    e->u8_set = true;
    e->held_x = nullptr;
    return XFR_OK;
}

xfr_status xfr_forward_u8(xfr_engine* e, const uint8_t* x_u8_dev, int32_t n, int32_t tensor_id, float* out_dev, void* stream)
{
    xfr_status st = require_u8(e);
    if (st != XFR_OK) return st;
    Scoped<bool> u8(e->u8_on, true);
    return xfr_forward(e, reinterpret_cast<const float*>(x_u8_dev), n, tensor_id, out_dev, stream);
}

xfr_status xfr_triplet_contrastive_u8(xfr_engine* e, const uint8_t* probes_u8_dev, const uint8_t* gallery_u8_dev, int32_t n, int32_t encode_tensor, float scale,
                                      float percentile, float* sal_dev, void* stream, int32_t inputs_ready)
{
    xfr_status st = require_u8(e);
    if (st != XFR_OK) return st;
    Scoped<bool> u8(e->u8_on, true);
    return xfr_triplet_contrastive(e, reinterpret_cast<const float*>(probes_u8_dev), reinterpret_cast<const float*>(gallery_u8_dev), n, encode_tensor, scale,
                                   percentile, sal_dev, stream, inputs_ready);
}

// Fresh uint8 images in HOST memory, every call (demo/test_whitebox.py:124-133: every call brings new images): the engine copies them itself -- its own
// copy stream, one device staging buffer per forward slot -- and orders the forwards behind THAT copy instead of behind the caller's stream, so the
// copy, the preprocessing and the forwards of call i + 1 overlap the sweep of call i without the caller promising anything about residency.
xfr_status xfr_triplet_contrastive_u8_host(xfr_engine* e, const uint8_t* probes_u8_host, const uint8_t* gallery_u8_host, int32_t n, int32_t encode_tensor,
                                           float scale, float percentile, float* sal_dev, void* stream)
{
    xfr_status st = require_u8(e);
    if (st != XFR_OK) return st;
    if (!probes_u8_host || !gallery_u8_host) return fail(XFR_INVALID_ARG, "null argument");
    if (n < 1 || 2 * n > e->max_batch) return fail(XFR_INVALID_ARG, "triplet batch %d needs max_batch >= %d (the gallery forward runs 2n images)", n, 2 * n);
    HIP_TRY(hipSetDevice(e->device));
    {
        xfr_status es = ensure_streams(e);
        if (es != XFR_OK) return es;
    }
    const size_t img = (size_t)e->u8_pre.channels * e->tens[0].HW();
    const size_t need = (size_t)(e->max_batch + e->max_batch / 2 + 1) * img;
    if (!e->s_copy) XFR_TRY(e->s_copy.create());
    // the slot the call below will take (xfr_triplet_contrastive: seq % n_slots when pipelined)
    const int slot = (e->pipeline && !e->profile_on) ? (int)(e->seq % e->n_slots) : 0;
    if (e->u8_stage[slot].cap < need) {
        for (int i = 0; i < 3; ++i) {
            if (e->u8_stage[i]) { HIP_TRY(hipDeviceSynchronize()); e->u8_stage[i].reset(); e->stage_busy[i] = false; }
        }
        DevBuf<uint8_t> stage[3];
        Event copied[3], stage_a[3], stage_b[3];
        for (int i = 0; i < 3; ++i) {
            XFR_TRY(stage[i].alloc(need));
            if (!e->ev_copied[i]) {
                XFR_TRY(copied[i].create());
                XFR_TRY(stage_a[i].create());
                XFR_TRY(stage_b[i].create());
            }
        }
        for (int i = 0; i < 3; ++i) {
            e->u8_stage[i] = std::move(stage[i]);
            if (!e->ev_copied[i]) { e->ev_copied[i] = std::move(copied[i]); e->ev_stage_a[i] = std::move(stage_a[i]); e->ev_stage_b[i] = std::move(stage_b[i]); }
        }
    }
    if (e->stage_busy[slot]) {                 // the forwards that last read this staging buffer
        HIP_TRY(hipStreamWaitEvent(e->s_copy, e->ev_stage_a[slot], 0));
        HIP_TRY(hipStreamWaitEvent(e->s_copy, e->ev_stage_b[slot], 0));
    }
    uint8_t* gal = e->u8_stage[slot];
    uint8_t* pro = gal + (size_t)2 * n * img;
    HIP_TRY(hipMemcpyAsync(gal, gallery_u8_host, (size_t)2 * n * img, hipMemcpyHostToDevice, e->s_copy));
    HIP_TRY(hipMemcpyAsync(pro, probes_u8_host, (size_t)n * img, hipMemcpyHostToDevice, e->s_copy));
    HIP_TRY(hipEventRecord(e->ev_copied[slot], e->s_copy));
    e->last_copied = e->ev_copied[slot];
    Scoped<bool> u8(e->u8_on, true);
    return triplet_contrastive(e, reinterpret_cast<const float*>(pro), reinterpret_cast<const float*>(gal), n, encode_tensor, scale, percentile, sal_dev,
                               stream, 0, TAIL_V6, e->ev_copied[slot], slot);
}

xfr_status xfr_engine_wait_inputs_copied(xfr_engine* e)
{
    if (!e) return fail(XFR_INVALID_ARG, "null engine");
    if (e->last_copied) HIP_TRY(hipEventSynchronize(e->last_copied));
    return XFR_OK;
}

xfr_status xfr_engine_set_epilogue_fusion(xfr_engine* e, int32_t enable)
{
    if (!e) return fail(XFR_INVALID_ARG, "null engine");
    e->fuse_gemm_epilogue = (enable & 1) != 0;
    e->fuse_fwd_only = (enable & 1) != 0;
    e->fuse_probe_fwd = (enable & 2) != 0 && (enable & 4) == 0;     // a dual launch needs the compiled epilogue
    e->interpret_chains = (enable & 4) != 0;
    // bit 3 (tests): the max-pool + average-pool pair of Light-CNN keeps its separate forward kernels and VJP launches.  The backward
    // schedules are built with or without the pair's chain head: drop the cached ones when the switch moves.
    const bool pools = (enable & 1) != 0 && (enable & 8) == 0;
    if (pools != e->fuse_pools) e->plans.clear();
    e->fuse_pools = pools;
    {
        const bool avgup = (enable & 1) != 0 && (enable & 64) == 0;   // bit 6 (tests): the down-sampling blocks' shortcut VJP as separate launches
        if (avgup != e->fuse_avgup) e->plans.clear();
        e->fuse_avgup = avgup;
    }
    {
        const bool branch = (enable & 1) != 0 && (enable & 128) == 0;   // bit 7 (tests): the main path's chain of a projection-shortcut block as its own launch
        if (branch != e->fuse_branch) e->plans.clear();
        e->fuse_branch = branch;
    }
    e->pair_tiles = (enable & 32) == 0;           // bit 5 (A/B measurements): tile order of the two-stream backward GEMMs as before round 4
    e->hoist_shortcut = (enable & 256) == 0;      // bit 8 (tests, A/B): the down-sampling blocks' shortcut in program order, their residual add as its own launch
    e->direct_stem = (enable & 16) == 0;          // bit 4 (tests): the first layer of Light-CNN through the GEMM like every other convolution
    e->overlap_phases = (enable & 512) == 0;      // bit 9 (tests, A/B): the phase launches of a strided KxK layer's backward-data pass one after another on the sweep's stream
    e->depthwise_valu = (enable & 1024) == 0;     // bit 10 (tests, A/B): depthwise launches stay on configuration 13 (conv_group.hip) instead of 14 (conv_depthwise.hip)
    e->held_x = nullptr;
    for (auto& p : e->plans) p.lean_state = -1;   // the lean tables follow the probe forward's fusion decisions
    return XFR_OK;
}

xfr_status xfr_engine_hold_forward(xfr_engine* e, int32_t hold)
{
    if (!e) return fail(XFR_INVALID_ARG, "null engine");
    e->hold_forward = hold != 0;
    e->held_x = nullptr;
    return XFR_OK;
}

xfr_status xfr_engine_set_tail_balance(xfr_engine* e, int32_t enable)
{
    if (!e) return fail(XFR_INVALID_ARG, "null engine");
    e->tail_balance = enable != 0;
    return XFR_OK;
}

xfr_status xfr_engine_set_split_gemm(xfr_engine* e, int32_t mode)
{
    if (!e) return fail(XFR_INVALID_ARG, "null engine");
    if (mode < 0 || mode > 7) return fail(XFR_INVALID_ARG, "xfr_engine_set_split_gemm: mode 0 (off), 1 (forward convolutions), 2 (backward-data GEMMs), 3 (both); + 4: whatever the launch's grid");
    e->split_mask = mode & 3;
    e->split_any_grid = (mode & 4) != 0;
    e->held_x = nullptr;
    presplit_weights(e);               // planes of the packs the new mode adds
    return XFR_OK;
}

xfr_status xfr_engine_split_gemm_stats(xfr_engine* e, int64_t* launches)
{
    if (!e || !launches) return fail(XFR_INVALID_ARG, "null argument");
    *launches = conv_gemm_split_launches();       // process-wide: the kernel's launch counter is not per engine
    return XFR_OK;
}

xfr_status xfr_engine_set_lean(xfr_engine* e, int32_t enable)
{
    if (!e) return fail(XFR_INVALID_ARG, "null engine");
    e->lean = enable != 0;
    e->held_x = nullptr;
    return XFR_OK;
}

xfr_status xfr_engine_lean_stats(xfr_engine* e, int64_t* dual_launches)
{
    if (!e || !dual_launches) return fail(XFR_INVALID_ARG, "null argument");
    *dual_launches = e->lean_launches;
    return XFR_OK;
}

xfr_status xfr_engine_set_forward_split(xfr_engine* e, int32_t enable)
{
    if (!e) return fail(XFR_INVALID_ARG, "null engine");
    e->split_forward = enable != 0;
    return XFR_OK;
}

xfr_status xfr_engine_set_pipeline(xfr_engine* e, int32_t enable)
{
    if (!e) return fail(XFR_INVALID_ARG, "null engine");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    const bool three = enable > 0 && (enable & 4) != 0;
    // the slots' forward regions, argmax bytes, seed buffers and events: built together, committed together (slot 0's region and bytes are the
    // workspace's own); seedbuf[i] stands for slot i
    const int slots = enable ? (three ? 3 : 2) : 0;
    DevBuf<float> region[3], seed[3];
    DevBuf<uint8_t> idx[3];
    Event done[3];
    for (int i = 1; i < slots; ++i) {
        if (e->seedbuf[i]) continue;
        XFR_TRY(region[i].alloc(e->fwd_region_floats));
        XFR_TRY(idx[i].alloc(e->idx_bytes));
    }
    for (int i = 0; i < slots; ++i) {
        if (e->seedbuf[i]) continue;
        XFR_TRY(seed[i].alloc(2 * (size_t)e->max_batch * e->max_per_n()));
        XFR_TRY(done[i].create());
    }
    for (int i = 0; i < slots; ++i) {
        if (e->seedbuf[i]) continue;
        if (i > 0) { e->fwd_ws[i] = std::move(region[i]); e->fwd_idx[i] = std::move(idx[i]); }
        e->seedbuf[i] = std::move(seed[i]); e->ev_slot_done[i] = std::move(done[i]);
    }
    if (enable) { xfr_status es = ensure_streams(e); if (es != XFR_OK) return es; }
    e->pipeline = enable != 0;
    e->pipeline_all = enable > 0 && (enable & 2) != 0;
    e->n_slots = three ? 3 : 2;
    e->slot_pending[0] = e->slot_pending[1] = e->slot_pending[2] = false;
    e->seq = 0;
    return XFR_OK;
}

xfr_status xfr_mwp_to_saliency(xfr_engine* e, const float* pooled_dev, int32_t n, int32_t h, int32_t w, float* sal_dev, void* stream)
{
    if (!e || !pooled_dev || !sal_dev) return fail(XFR_INVALID_ARG, "null argument");
    if (n < 1 || (size_t)n * h * w > 2 * (size_t)e->max_batch * e->tens[1].HW())
        return fail(XFR_INVALID_ARG, "xfr_mwp_to_saliency: %d maps of %dx%d exceed the engine's scratch", n, h, w);
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    launch_saliency_blur(pooled_dev, e->ws + e->blur_b_off, sal_dev, n, h, w, e->eps, s);
    HIP_TRY(hipGetLastError());
    return XFR_OK;
}

xfr_status xfr_mwp_to_saliency_u8(xfr_engine* e, const float* pooled_dev, const uint8_t* levels_dev, int32_t n, int32_t h, int32_t w,
                                  uint8_t* sal_dev, void* stream)
{
    if (!e || !sal_dev) return fail(XFR_INVALID_ARG, "xfr_mwp_to_saliency_u8: null argument");
    if ((pooled_dev != nullptr) == (levels_dev != nullptr))
        return fail(XFR_INVALID_ARG, "xfr_mwp_to_saliency_u8: exactly one of pooled_dev and levels_dev must be given, got %s", pooled_dev ? "both" : "neither");
    if (n < 1 || h < 1 || w < 1 || (long)h * w > U8_TAIL_MAX_HW)
        return fail(XFR_INVALID_ARG, "xfr_mwp_to_saliency_u8: n %d, h %d, w %d: need n, h, w >= 1 and h * w <= %d", n, h, w, U8_TAIL_MAX_HW);
    HIP_TRY(hipSetDevice(e->device));
    launch_u8_tail(pooled_dev, levels_dev, false, sal_dev, nullptr, n, h, w, e->eps, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return XFR_OK;
}

xfr_status xfr_firing_count(xfr_engine* e, int32_t seed_tensor, int32_t* n_firings)
{
    if (!e || !n_firings) return fail(XFR_INVALID_ARG, "null argument");
    if (e->need_dirty) compute_need(e);
    BwdPlan* plan = nullptr;
    xfr_status st = get_plan(e, seed_tensor, &plan);
    if (st != XFR_OK) return st;
    *n_firings = plan->n_firings;
    return XFR_OK;
}

xfr_status xfr_firing_kinds(xfr_engine* e, int32_t seed_tensor, int32_t* kinds, int32_t capacity)
{
    if (!e || !kinds) return fail(XFR_INVALID_ARG, "null argument");
    if (e->need_dirty) compute_need(e);
    BwdPlan* plan = nullptr;
    xfr_status st = get_plan(e, seed_tensor, &plan);
    if (st != XFR_OK) return st;
    if (capacity < plan->n_firings) return fail(XFR_INVALID_ARG, "need room for %d kinds", plan->n_firings);
    for (int i = 0; i < plan->n_firings; ++i) kinds[i] = plan->firing_kinds[i];
    return XFR_OK;
}

xfr_status xfr_engine_set_inputs_ready(xfr_engine* e, int32_t ready)
{
    if (!e) return fail(XFR_INVALID_ARG, "null engine");
    e->inputs_ready = ready != 0;
    return XFR_OK;
}

xfr_status xfr_engine_set_trace(xfr_engine* e, int32_t enable)
{
    if (!e) return fail(XFR_INVALID_ARG, "null engine");
    e->trace_on = enable ? 1 : 0;
    return XFR_OK;
}

xfr_status xfr_engine_trace_size(xfr_engine* e, int32_t* n_firings)
{
    if (!e || !n_firings) return fail(XFR_INVALID_ARG, "null argument");
    *n_firings = e->last_trace_firings;
    return XFR_OK;
}

xfr_status xfr_engine_get_trace(xfr_engine* e, double* sums, int32_t* kinds, int32_t capacity)
{
    if (!e || !sums) return fail(XFR_INVALID_ARG, "null argument");
    const int nf = e->last_trace_firings, SB = e->last_trace_sb;
    if (capacity < nf * SB) return fail(XFR_INVALID_ARG, "trace needs %d doubles", nf * SB);
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(sums, e->dbl_ws + 2 * e->max_batch, sizeof(double) * (size_t)nf * SB, hipMemcpyDeviceToHost));
    if (kinds) for (int i = 0; i < nf; ++i) kinds[i] = e->last_trace_kinds[i];
    return XFR_OK;
}

xfr_status xfr_engine_profile_csv(xfr_engine* e, const char* path)
{
    if (!e) return fail(XFR_INVALID_ARG, "null engine");
    e->profile_csv = path ? path : "";
    return XFR_OK;
}

xfr_status xfr_chain_epilogue_stats(int64_t* compiled_launches, int64_t* interpreted_launches, int32_t* n_signatures)
{
    long c = 0, i = 0;
    conv_gemm_chain_launch_counts(&c, &i);
    if (compiled_launches) *compiled_launches = c;
    if (interpreted_launches) *interpreted_launches = i;
    if (n_signatures) *n_signatures = conv_gemm_num_chain_sigs();
    return XFR_OK;
}

xfr_status xfr_elementwise_launch_stats(int64_t* counts, int32_t capacity, int32_t* n_variants)
{
    const int n = elementwise_num_variants();
    if (n_variants) *n_variants = n;
    if (capacity < 0 || (capacity > 0 && !counts)) return fail(XFR_INVALID_ARG, "xfr_elementwise_launch_stats: bad arguments");
    for (int i = 0; i < n && i < capacity; ++i) counts[i] = elementwise_variant_launches(i);
    return XFR_OK;
}

const char* xfr_elementwise_variant_name(int32_t i) { return elementwise_variant_name(i); }

xfr_status xfr_engine_memory(xfr_engine* e, size_t* weight_bytes, size_t* workspace_bytes)
{
    if (!e) return fail(XFR_INVALID_ARG, "null engine");
    if (weight_bytes) *weight_bytes = e->arena_floats * sizeof(float);
    if (workspace_bytes) *workspace_bytes = e->ws_floats * sizeof(float) + e->idx_bytes;
    return XFR_OK;
}

xfr_status xfr_engine_set_profile(xfr_engine* e, int32_t enable)
{
    if (!e) return fail(XFR_INVALID_ARG, "null engine");
    e->profile_on = enable ? 1 : 0;
    return XFR_OK;
}

xfr_status xfr_engine_get_profile(xfr_engine* e, double* gemm_ms, int64_t* gemm_launches, double* gemm_flops)
{
    if (!e) return fail(XFR_INVALID_ARG, "null engine");
    if (gemm_ms) *gemm_ms = e->last_gemm_ms;
    if (gemm_launches) *gemm_launches = e->last_gemm_launches;
    if (gemm_flops) *gemm_flops = e->last_gemm_flops;
    return XFR_OK;
}

xfr_status xfr_engine_get_profile_by_kernel(xfr_engine* e, double* gemm_ms, int64_t* gemm_launches, double* gemm_flops)
{
    if (!e || !gemm_ms || !gemm_launches || !gemm_flops) return fail(XFR_INVALID_ARG, "null argument");
    for (int q = 0; q < 2; ++q) { gemm_ms[q] = e->fam_ms[q]; gemm_launches[q] = e->fam_launches[q]; gemm_flops[q] = e->fam_flops[q]; }
    return XFR_OK;
}

}  // extern "C"
