// plan.hip -- the static analysis of a layer program, done once at engine creation.  Device-free: nothing here calls the runtime or launches a kernel
// (xfr_plan_describe runs all of it without a GPU).
//
// What the reference does with forward hooks, pre-forward hooks, tensor hooks and a freshly recorded autograd
// graph on every call (whitebox.py:306-437, :482-504) is done here once:
//   * shape inference over the static layer program;
//   * the hook table: which (module call, input) hooks sit on which tensor, in registration order, with the
//     in-place-ReLU placement and the late-binding (a, x) of two-input Add modules;
//   * a static analysis of the 'positive_activation' pass (whitebox.py:315-330): for every tensor whether its
//     positive-pass value equals the true value (EQ), equals relu(true value) (RELU) or has to be computed
//     (OTHER), so that X is only materialised where it differs from A;
//   * the layout of the workspace and of the parameter arena;
//   * the backward schedule: GEMMs for conv/linear VJPs with relu(W), and every elementwise step between two
//     GEMMs (tensor hooks, ReLU masks, BatchNorm / Multiply VJPs) as one EwChain launch (plan_fuse.hip fuses across them).
#include "engine_internal.h"

namespace xfr {
namespace {

bool is_hooked(int kind) { return kind >= XFR_OP_CONV && kind <= XFR_OP_SPLIT; }

int hook_action(int mode, int kind)
{
    switch (mode) {
        case XFR_MODE_AFFINEONLY: return is_affine_name(kind) ? HOOK_DIV : HOOK_PASS;
        case XFR_MODE_AFFINEONLY_WITH_PRIOR: return is_affine_name(kind) ? HOOK_DIV : HOOK_RELU;
        default: return HOOK_DIV;   // 'norelu' without priors and 'all' (whitebox.py:416-428)
    }
}

int pool_out(int in, int k, int s, int p, bool ceil_mode)
{
    int num = in + 2 * p - k;
    int o = (ceil_mode ? (num + s - 1) / s : num / s) + 1;
    if (ceil_mode && (o - 1) * s >= in + p) --o;   // last window must start inside the (left-padded) input
    return o;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------
xfr_status build(xfr_engine* e, const xfr_op_desc* ops, int n_ops)
{
    e->tens.resize(n_ops + 1);
    e->ops.resize(n_ops);
    Tensor& in = e->tens[0];
    in.C = e->in_c; in.H = e->in_h; in.W = e->in_w;
    in.pstate = PS_EQ;
    for (int k = 0; k < n_ops; ++k) {
        OpRec& o = e->ops[k];
        o.d = ops[k];
        const xfr_op_desc& d = o.d;
        if (d.out != k + 1) return fail(XFR_INVALID_ARG, "op %d: out tensor id must be %d (got %d)", k, k + 1, d.out);
        if (d.in0 < 0 || d.in0 > k) return fail(XFR_INVALID_ARG, "op %d: bad in0 %d", k, d.in0);
        const bool two = (d.kind == XFR_OP_ADD || d.kind == XFR_OP_G_ADD);
        if (two && (d.in1 < 0 || d.in1 > k)) return fail(XFR_INVALID_ARG, "op %d: bad in1 %d", k, d.in1);
        auto chkw = [&](int w) { return w >= -1 && w < e->n_weights; };
        if (!chkw(d.w_weight) || !chkw(d.w_bias) || !chkw(d.w_mean) || !chkw(d.w_var))
            return fail(XFR_INVALID_ARG, "op %d: weight index out of range", k);
        const Tensor& a = e->tens[d.in0];
        Tensor& t = e->tens[d.out];
        t.producer = k;
        e->tens[d.in0].consumers.push_back(k);
        if (two) e->tens[d.in1].consumers.push_back(k);
        switch (d.kind) {
            case XFR_OP_CONV:
            case XFR_OP_LINEAR: {
                if (d.cout <= 0 || d.kh <= 0 || d.kw <= 0 || d.stride <= 0 || d.pad < 0 || d.w_weight < 0)
                    return fail(XFR_INVALID_ARG, "op %d: bad conv/linear geometry", k);
                if (d.kind == XFR_OP_LINEAR && (d.kh != a.H || d.kw != a.W || d.pad != 0))
                    return fail(XFR_INVALID_ARG, "op %d: linear kernel must equal the input extent %dx%d", k, a.H, a.W);
                // grouped convolution: `groups` travels in the ceil_mode slot (0 and 1: an ordinary convolution)
                if (d.ceil_mode < 0) return fail(XFR_INVALID_ARG, "op %d: groups must be >= 1 (got %d)", k, d.ceil_mode);
                const int G = d.ceil_mode > 1 ? d.ceil_mode : 1;
                if (G > 1) {
                    if (d.kind == XFR_OP_LINEAR) return fail(XFR_UNSUPPORTED_LAYER, "op %d: groups %d on a Linear layer is not supported", k, G);
                    if (k == 0)
                        return fail(XFR_UNSUPPORTED_LAYER, "op %d: groups %d on the first layer is not supported (the image stem has its own paths)", k, G);
                    if (a.C % G) return fail(XFR_INVALID_ARG, "op %d: %d input channels are not divisible by groups %d", k, a.C, G);
                    if (d.cout % G) return fail(XFR_INVALID_ARG, "op %d: %d output channels are not divisible by groups %d", k, d.cout, G);
                }
                o.groups = G;
                t.C = d.cout;
                t.H = (a.H + 2 * d.pad - d.kh) / d.stride + 1;
                t.W = (a.W + 2 * d.pad - d.kw) / d.stride + 1;
                if (t.H <= 0 || t.W <= 0) return fail(XFR_INVALID_ARG, "op %d: empty conv output", k);
                if (d.stride > 1 && !(d.kh == 1 && d.kw == 1) && k != 0) {
                    // backward-data by phases (PhaseRec): padding <= kernel - stride keeps every phase's leading padding non-negative
                    if (d.pad > d.kh - d.stride || d.pad > d.kw - d.stride)
                        return fail(XFR_UNSUPPORTED_LAYER, "op %d: a strided %dx%d convolution behind the first layer needs pad <= kernel - stride on "
                                    "each axis (stride %d, pad %d): its backward-data pass runs by phases", k, d.kh, d.kw, d.stride, d.pad);
                    const int s = d.stride, p = d.pad;
                    for (int r = 0; r < s && r < d.kh; ++r)
                        for (int c = 0; c < s && c < d.kw; ++c) {
                            PhaseRec ph;
                            ph.r = r; ph.c = c;
                            ph.ka = (d.kh - r + s - 1) / s; ph.kb = (d.kw - c + s - 1) / s;
                            ph.q0 = p > r ? (p - r + s - 1) / s : 0; ph.u0 = p > c ? (p - c + s - 1) / s : 0;
                            ph.ih0 = s * ph.q0 + r - p; ph.iw0 = s * ph.u0 + c - p;
                            if (ph.ih0 >= a.H || ph.iw0 >= a.W) continue;      // the phase's origin lies outside the map
                            ph.nq = (a.H - 1 - ph.ih0) / s + 1; ph.nu = (a.W - 1 - ph.iw0) / s + 1;
                            ph.K = d.cout / G * ph.ka * ph.kb;
                            ph.tap = G == 1 && (d.cout % 16 == 0) && (ph.ka * ph.kb <= 64);
                            o.phases.push_back(ph);
                        }
                }
                o.Cin = a.C; o.K = a.C / G * d.kh * d.kw; o.Kb = d.cout / G * d.kh * d.kw;      // of ONE group where the layer has groups
                t.nonneg = false; t.pstate = PS_OTHER;
                break;
            }
            case XFR_OP_BATCHNORM:
                if (d.w_weight < 0 || d.w_bias < 0 || d.w_mean < 0 || d.w_var < 0)
                    return fail(XFR_INVALID_ARG, "op %d: batchnorm needs weight, bias, running_mean, running_var", k);
                t.C = a.C; t.H = a.H; t.W = a.W; t.nonneg = false; t.pstate = PS_OTHER;
                break;
            case XFR_OP_RELU:
                t.C = a.C; t.H = a.H; t.W = a.W; t.nonneg = true; t.pstate = PS_EQ;
                if (d.inplace) {
                    if (e->tens[d.in0].consumers.size() != 1)
                        return fail(XFR_UNSUPPORTED_LAYER, "op %d: in-place ReLU on a tensor with other consumers", k);
                    t.alias = d.in0;
                }
                break;
            case XFR_OP_MAXPOOL:
                if (d.kh != d.kw || d.kh <= 0 || d.kh > 15 || d.stride <= 0) return fail(XFR_INVALID_ARG, "op %d: bad maxpool", k);
                t.C = a.C; t.H = pool_out(a.H, d.kh, d.stride, d.pad, d.ceil_mode != 0);
                t.W = pool_out(a.W, d.kw, d.stride, d.pad, d.ceil_mode != 0);
                t.nonneg = a.nonneg; t.pstate = a.nonneg ? PS_EQ : PS_RELU;
                break;
            case XFR_OP_AVGPOOL:
                if (d.kh != d.kw || d.kh <= 0 || d.stride <= 0 || d.pad != 0) return fail(XFR_INVALID_ARG, "op %d: bad avgpool", k);
                t.C = a.C; t.H = (a.H - d.kh) / d.stride + 1; t.W = (a.W - d.kw) / d.stride + 1;
                t.nonneg = a.nonneg; t.pstate = a.nonneg ? PS_EQ : PS_OTHER;
                if (d.kh == 1 && d.stride == 1) t.alias = d.in0;       // AvgPool2d(1, 1) (resnet.py:210): the identity -- same storage, no launch
                break;
            case XFR_OP_ADD:
            case XFR_OP_G_ADD: {
                const Tensor& b = e->tens[d.in1];
                if (a.C != b.C || a.H != b.H || a.W != b.W) return fail(XFR_INVALID_ARG, "op %d: add shape mismatch", k);
                t.C = a.C; t.H = a.H; t.W = a.W; t.nonneg = a.nonneg && b.nonneg;
                if (d.kind == XFR_OP_ADD) t.pstate = (a.nonneg && b.nonneg) ? PS_EQ : PS_OTHER;
                else t.pstate = (a.pstate == PS_EQ && b.pstate == PS_EQ) ? PS_EQ : PS_OTHER;
                break;
            }
            case XFR_OP_CONCAT:
                if (d.cout < 0) return fail(XFR_INVALID_ARG, "op %d: bad concat", k);
                t.C = a.C * (1 + d.cout); t.H = a.H; t.W = a.W; t.nonneg = a.nonneg; t.pstate = a.nonneg ? PS_EQ : PS_RELU;
                break;
            case XFR_OP_MULTIPLY:
                if (!(d.fparam > 0.f)) return fail(XFR_UNSUPPORTED_LAYER, "op %d: Multiply(n) needs n > 0", k);
                t.C = a.C; t.H = a.H; t.W = a.W; t.nonneg = a.nonneg; t.pstate = a.nonneg ? PS_EQ : PS_RELU;
                break;
            case XFR_OP_SPLIT:
                t.C = a.C; t.H = a.H; t.W = a.W; t.nonneg = a.nonneg; t.pstate = a.nonneg ? PS_EQ : PS_RELU;
                t.alias = d.in0;
                break;
            case XFR_OP_G_MAXHALVES:
                if (a.C % 2) return fail(XFR_INVALID_ARG, "op %d: max-of-halves needs an even channel count", k);
                t.C = a.C / 2; t.H = a.H; t.W = a.W; t.nonneg = a.nonneg; t.pstate = a.pstate;
                break;
            case XFR_OP_G_NORMALIZE:
                if (a.H != 1 || a.W != 1) return fail(XFR_UNSUPPORTED_LAYER, "op %d: normalize is only supported on N x C vectors", k);
                t.C = a.C; t.H = 1; t.W = 1; t.nonneg = false; t.pstate = (a.pstate == PS_EQ) ? PS_EQ : PS_OTHER;
                break;
            default:
                return fail(XFR_UNSUPPORTED_LAYER, "op %d: unsupported layer kind %d (Sigmoid/ELU/Tanh and friends are not "
                            "supported, see whitebox.py:403)", k, d.kind);
        }
        if (t.nonneg && t.pstate == PS_RELU) t.pstate = PS_EQ;
    }
    // an in-place ReLU overwrites its input: nothing else may read that tensor, before or after the ReLU in call order
    for (int k = 0; k < n_ops; ++k) {
        const xfr_op_desc& d = e->ops[k].d;
        if (d.kind == XFR_OP_RELU && d.inplace && e->tens[d.in0].consumers.size() != 1)
            return fail(XFR_UNSUPPORTED_LAYER, "op %d: in-place ReLU on tensor %d, which op %d also reads", k, d.in0,
                        e->tens[d.in0].consumers[e->tens[d.in0].consumers[0] == k ? 1 : 0]);
    }
    // hook table (registration order == call order)
    for (int k = 0; k < n_ops; ++k) {
        const xfr_op_desc& d = e->ops[k].d;
        if (!is_hooked(d.kind)) continue;
        const int nin = (d.kind == XFR_OP_ADD) ? 2 : 1;
        const int last_in = (nin == 2) ? d.in1 : d.in0;
        for (int j = 0; j < nin; ++j) {
            const int tin = (j == 0) ? d.in0 : d.in1;
            const int ht = (d.kind == XFR_OP_RELU && d.inplace) ? d.out : tin;
            Hook h; h.op = k; h.j = j; h.a_tensor = (d.kind == XFR_OP_RELU && d.inplace) ? d.out : last_in;
            e->tens[ht].hooks.push_back(h);
        }
    }
    e->is_hook_a.assign(e->tens.size(), 0);
    for (auto& x : e->tens)
        for (const Hook& h : x.hooks) e->is_hook_a[h.a_tensor] = 1;
    // forward fusion: <BatchNorm | Add | functional add> followed by an in-place ReLU on its output
    for (int k = 0; k + 1 < n_ops; ++k) {
        const xfr_op_desc& d = e->ops[k].d;
        const xfr_op_desc& nx = e->ops[k + 1].d;
        if ((d.kind == XFR_OP_BATCHNORM || d.kind == XFR_OP_ADD || d.kind == XFR_OP_G_ADD) && nx.kind == XFR_OP_RELU &&
            nx.inplace && nx.in0 == d.out) {
            e->ops[k].fuse_relu = true;
            e->ops[k + 1].relu_fused_away = true;
        }
    }
    // MaxFeatureMap: Conv -> Split -> torch.max(halves) with single consumers all the way
    for (int k = 0; k + 2 < n_ops; ++k) {
        const xfr_op_desc& d = e->ops[k].d;
        if (d.kind != XFR_OP_CONV || (d.cout & 1) || e->tens[d.out].consumers.size() != 1) continue;
        const int k1 = e->tens[d.out].consumers[0];
        if (e->ops[k1].d.kind != XFR_OP_SPLIT || e->tens[e->ops[k1].d.out].consumers.size() != 1) continue;
        const int k2 = e->tens[e->ops[k1].d.out].consumers[0];
        if (e->ops[k2].d.kind != XFR_OP_G_MAXHALVES) continue;
        if (e->ops[k].groups > 1)
            return fail(XFR_UNSUPPORTED_LAYER, "op %d: groups %d on a MaxFeatureMap pair convolution (Conv -> Split -> max of halves) is not supported", k,
                        e->ops[k].groups);
        e->ops[k].pair = d.cout / 2;
        e->ops[k].pair_split = k1;
        e->ops[k].pair_max = k2;
    }
    return XFR_OK;
}

static void mark_need(xfr_engine* e, int t)
{
    Tensor& x = e->tens[t];
    if (x.pstate != PS_OTHER || x.need_pv) return;
    x.need_pv = true;
    if (x.producer < 0) return;
    const xfr_op_desc& d = e->ops[x.producer].d;
    if (!is_hooked(d.kind)) {   // glue consumes positive-pass values of its inputs
        mark_need(e, d.in0);
        if (d.kind == XFR_OP_G_ADD) mark_need(e, d.in1);
    }
}

void compute_need(xfr_engine* e)
{
    for (auto& t : e->tens) t.need_pv = false;
    for (size_t t = 0; t < e->tens.size(); ++t)
        for (const Hook& h : e->tens[t].hooks)
            if (hook_action(e->mode, e->ops[h.op].d.kind) == HOOK_DIV) {
                // x of the hook = relu(positive-pass value of the call's LAST input); for an in-place ReLU the call's input
                const xfr_op_desc& d = e->ops[h.op].d;
                const int xt = (d.kind == XFR_OP_ADD) ? d.in1 : d.in0;
                mark_need(e, xt);
            }
    e->need_dirty = false;
    e->plans.clear();
    e->stat_plan = nullptr;       // the cached descriptor table belonged to one of those plans
}

// ---------------------------------------------------------------------------------------------------------------
xfr_status layout_workspace(xfr_engine* e)
{
    const size_t B = (size_t)e->max_batch;
    for (auto& x : e->tens)
        if (2 * B * (size_t)x.per_n() * sizeof(float) >= (1ull << 31))
            return fail(XFR_INVALID_ARG, "max_batch %d makes a tensor exceed 2 GiB (32-bit buffer offsets)", e->max_batch);
    size_t off = 0;
    auto take = [&](size_t n) { size_t o = off; off += align_up(n, 64); return o; };
    e->x_off = take(B * e->tens[0].per_n());
    // ConcatChannels (resnet.py:210-213) pads the pooled shortcut with zero channels.  In CNHW a channel prefix is a storage prefix for every
    // batch size, so the pooled tensor lives INSIDE the padded one: the average pool writes it there and the padding is one fill, no copy.
    for (auto& o : e->ops) {
        if (o.d.kind != XFR_OP_CONCAT) continue;
        Tensor& in = e->tens[o.d.in0];
        if (in.alias >= 0 || e->tens[o.d.out].alias >= 0 || in.consumers.size() != 1 || in.producer < 0 ||
            e->ops[in.producer].d.kind != XFR_OP_AVGPOOL)
            continue;
        in.prefix_of = o.d.out;
    }
    for (size_t t = 0; t < e->tens.size(); ++t) {
        Tensor& x = e->tens[t];
        if (x.alias < 0 && x.prefix_of < 0) x.t_off = take(B * x.per_n());
    }
    for (auto& x : e->tens)
        if (x.prefix_of >= 0) x.t_off = e->tens[x.prefix_of].t_off;
    e->t_region_floats = off;
    for (size_t t = 0; t < e->tens.size(); ++t) {
        Tensor& x = e->tens[t];
        if (x.pstate == PS_OTHER) x.pv_off = take(B * x.per_n());
    }
    // normalize norms live in the forward region too (written by the forward, read by the backward)
    size_t misc = 0;
    size_t idxb = 0;
    for (auto& o : e->ops) {
        if (o.d.kind == XFR_OP_G_NORMALIZE) { o.norm_off = misc; misc += align_up(B, 64); }
        if (o.d.kind == XFR_OP_MAXPOOL) { o.idx_off = idxb; idxb += align_up(B * e->tens[o.d.out].per_n(), 256); }
    }
    e->misc_off = take(std::max<size_t>(misc, 64));
    take(4096);
    e->fwd_region_floats = off;
    e->g_begin = off;
    for (size_t t = 1; t < e->tens.size(); ++t) e->tens[t].g_off = take(2 * B * e->tens[t].per_n());
    e->g_end = off;
    e->seed_off = take(2 * B * e->max_per_n());
    const Tensor& t1 = e->tens[1];
    e->tap_off = take(2 * B * t1.per_n());
    e->pooled_off = take(2 * B * t1.HW());
    e->blur_a_off = take(2 * B * std::max(t1.HW(), 1));
    e->blur_b_off = take(2 * B * std::max(t1.HW(), 1));
    e->thr_off = take(B);
    take(4096);   // slack: vector loads of a tile's dead columns may run past the last tensor
    e->ws_floats = off;
    e->idx_bytes = std::max<size_t>(idxb, 256);
    return XFR_OK;
}

// parameter arena layout
xfr_status layout_arena(xfr_engine* e)
{
    size_t off = 0;
    auto take = [&](size_t n) { size_t o = off; off += align_up(n, 64); return (long)o; };
    for (size_t k = 0; k < e->ops.size(); ++k) {
        OpRec& o = e->ops[k];
        const xfr_op_desc& d = o.d;
        if ((d.kind == XFR_OP_CONV || d.kind == XFR_OP_LINEAR) && o.groups > 1) {
            // a grouped layer: the same set of packs in the per-group layout of conv_group.hip (common.h: group_pack_floats), no tap-major order
            const int Ci = o.Cin / o.groups, Co = d.cout / o.groups;
            o.Kf = o.K;
            o.w_true = take(group_pack_floats(o.groups, Co, o.K));
            o.w_pos = take(group_pack_floats(o.groups, Co, o.K));
            if (o.phases.empty()) {
                o.w_bwd = take(group_pack_floats(o.groups, Ci, o.Kb));
                o.w_bwd_true = take(group_pack_floats(o.groups, Ci, o.Kb));
            }
            for (PhaseRec& ph : o.phases) {
                ph.w_bwd = take(group_pack_floats(o.groups, Ci, ph.K));
                ph.w_bwd_true = take(group_pack_floats(o.groups, Ci, ph.K));
            }
            if (d.w_bias >= 0) { o.b_true = take(d.cout); o.b_pos = take(d.cout); }
        } else if (d.kind == XFR_OP_CONV || d.kind == XFR_OP_LINEAR) {
            o.ldw = (int)align_up(d.cout, 128);
            o.tap_fwd = (d.kh * d.kw > 1) && (o.Cin % 16 == 0) && (d.kh * d.kw <= 64);
            o.tap_bwd = (d.kh * d.kw > 1) && (d.cout % 16 == 0) && (d.kh * d.kw <= 64);
            o.tap4_fwd = (d.kh * d.kw > 1) && (o.Cin == 3 || o.Cin == 4) && (d.kh * d.kw <= 60);
            o.Kf = o.tap4_fwd ? 4 * d.kh * d.kw : o.K;
            o.w_true = take(align_up(o.Kf, 32) * o.ldw);
            o.w_pos = take(align_up(o.Kf, 32) * o.ldw);
            if (k != 0) {
                o.ldb = (int)align_up(o.Cin, 128);
                if (o.phases.empty()) {
                    o.w_bwd = take(align_up(o.Kb, 32) * o.ldb);
                    o.w_bwd_true = take(align_up(o.Kb, 32) * o.ldb);
                }
                for (PhaseRec& ph : o.phases) {      // a strided KxK layer: one flipped sub-kernel pack per phase instead of the whole kernel's
                    ph.w_bwd = take(align_up(ph.K, 32) * o.ldb);
                    ph.w_bwd_true = take(align_up(ph.K, 32) * o.ldb);
                }
            }
            if (d.w_bias >= 0) { o.b_true = take(d.cout); o.b_pos = take(d.cout); }
        } else if (d.kind == XFR_OP_BATCHNORM) {
            const int C = e->tens[d.out].C;
            o.bn_alpha_t = take(C); o.bn_beta_t = take(C); o.bn_alpha_p = take(C); o.bn_beta_p = take(C); o.bn_beta_pb = take(C);
        }
    }
    e->arena_floats = std::max<size_t>(off, 64);
    return XFR_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// backward schedule
static bool unary_elementwise(int kind)
{
    return kind == XFR_OP_RELU || kind == XFR_OP_BATCHNORM || kind == XFR_OP_MULTIPLY || kind == XFR_OP_SPLIT;
}

static xfr_status make_plan(xfr_engine* e, int seed_tensor, BwdPlan& plan, bool plain)
{
    plan.plain = plain;
    const int nt = (int)e->tens.size();
    plan.seed_tensor = seed_tensor;
    plan.mode = e->mode;
    plan.steps.clear();
    // reachability: every op propagates to all of its inputs
    std::vector<char> reach(nt, 0);
    reach[seed_tensor] = 1;
    for (int k = e->tens[seed_tensor].producer; k >= 0; --k) {
        const xfr_op_desc& d = e->ops[k].d;
        if (!reach[d.out]) continue;
        reach[d.in0] = 1;
        if (d.kind == XFR_OP_ADD || d.kind == XFR_OP_G_ADD) reach[d.in1] = 1;
    }
    // number of gradient contributors per tensor
    std::vector<int> contrib(nt, 0);
    for (int k = 0; k <= e->tens[seed_tensor].producer; ++k) {
        const xfr_op_desc& d = e->ops[k].d;
        if (!reach[d.out]) continue;
        contrib[d.in0]++;
        if (d.kind == XFR_OP_ADD || d.kind == XFR_OP_G_ADD) contrib[d.in1]++;
    }
    // firing order (reference): descending producer index, registration order within a tensor; image last
    std::vector<std::vector<int>> slot(nt);
    plan.firing_kinds.clear();
    plan.firing_ops.clear();
    plan.firing_tensor.clear();
    for (int k = e->tens[seed_tensor].producer; k >= 0; --k) {
        const int t = e->ops[k].d.out;
        if (!reach[t]) continue;
        for (const Hook& h : e->tens[t].hooks) {
            if (e->ops[h.op].d.out > seed_tensor) { slot[t].push_back(-1); continue; }   // call beyond the seed
            slot[t].push_back((int)plan.firing_kinds.size());
            plan.firing_kinds.push_back(e->ops[h.op].d.kind);
            plan.firing_ops.push_back(h.op);
            plan.firing_tensor.push_back(t);
        }
    }
    plan.n_firings = (int)plan.firing_kinds.size();   // (+1 for the image hook of op 0, which is not computed)

    std::vector<char> written(nt, 0), hooks_done(nt, 0), op_done(e->ops.size(), 0);
    written[seed_tensor] = 1;

    auto append_hooks = [&](BwdStep& st, int t) -> bool {
        const Tensor& x = e->tens[t];
        for (size_t i = 0; i < x.hooks.size(); ++i) {
            const Hook& h = x.hooks[i];
            if (slot[t][i] < 0) continue;   // hook of a call that lies beyond the seed tensor
            if (plain) continue;            // plain gradients: the _savegrad hooks only record
            const xfr_op_desc& hd = e->ops[h.op].d;
            BwdStep::Sym sy;
            sy.type = EW_HOOK;
            sy.action = hook_action(e->mode, hd.kind);
            sy.t0 = h.a_tensor;
            const int xt = (hd.kind == XFR_OP_ADD) ? hd.in1 : hd.in0;
            sy.x_t = (e->tens[xt].pstate == PS_OTHER) ? xt : -1;   // -1: x == a
            sy.f = 0.f; sy.op = h.op; sy.slot = slot[t][i]; sy.tap = false;
            st.chain.push_back(sy);
        }
        hooks_done[t] = 1;
        return true;
    };

    for (int k = e->tens[seed_tensor].producer; k >= 1; --k) {
        if (op_done[k]) continue;
        const int t0 = e->ops[k].d.out;
        if (!reach[t0]) continue;
        BwdStep ew;
        ew.kind = ST_EW;
        ew.src_t = t0;
        ew.ew_t = t0;
        if (!hooks_done[t0]) append_hooks(ew, t0);
        int cur_op = k;
        int cur_t = t0;
        bool emitted = false;
        while (true) {
            const xfr_op_desc& d = e->ops[cur_op].d;
            if (!unary_elementwise(d.kind)) break;
            // VJP of the elementwise op
            BwdStep::Sym sy;
            sy.action = 0; sy.x_t = -1; sy.f = 0.f; sy.op = cur_op; sy.slot = -1; sy.tap = false; sy.t0 = -1;
            bool has = true;
            if (d.kind == XFR_OP_RELU) { sy.type = EW_MASK; sy.t0 = d.out; }
            else if (d.kind == XFR_OP_BATCHNORM) { sy.type = EW_SCALE_C; }
            else if (d.kind == XFR_OP_MULTIPLY) { sy.type = EW_SCALE; sy.f = d.fparam; }
            else has = false;
            if (has) ew.chain.push_back(sy);
            op_done[cur_op] = 1;
            const int ti = d.in0;
            if (ti == 0) {   // reached the image: nothing below
                emitted = true;   // nothing to store
                ew.chain.clear();
                break;
            }
            const bool single = (contrib[ti] == 1);
            const bool room = (ew.chain.size() + e->tens[ti].hooks.size() + 2 <= XFR_MAX_EW_STEPS);
            if (single && room && ti != 1) {
                append_hooks(ew, ti);
                cur_t = ti;
                cur_op = e->tens[ti].producer;
                if (op_done[cur_op]) break;
                continue;
            }
            if (single && room && ti == 1) {
                // tensor 1 = output of the first layer: its last hook is P[-2] (whitebox.py:499); stop here
                append_hooks(ew, ti);
                for (int q = (int)ew.chain.size() - 1; q >= 0; --q)
                    if (ew.chain[q].type == EW_HOOK) { ew.chain[q].tap = true; break; }
                ew.dst_t = 1; ew.accumulate = 0;
                plan.steps.push_back(ew);
                return XFR_OK;
            }
            // store into G[ti] (possibly accumulating); its hooks fire later when its producer is visited
            ew.dst_t = ti; ew.accumulate = written[ti] ? 1 : 0;
            written[ti] = 1;
            plan.steps.push_back(ew);
            emitted = true;
            break;
        }
        if (emitted) continue;
        // cur_t's producer (cur_op) is not elementwise (or already done): flush the chain in place, then its VJP
        if (cur_t == 1) {
            // hooks of tensor 1 were appended by a chain that started above; mark the tap
            for (int q = (int)ew.chain.size() - 1; q >= 0; --q)
                if (ew.chain[q].type == EW_HOOK) { ew.chain[q].tap = true; break; }
            ew.dst_t = 1; ew.accumulate = 0;
            plan.steps.push_back(ew);
            return XFR_OK;
        }
        if (!ew.chain.empty() || cur_t != t0) {
            ew.dst_t = cur_t; ew.accumulate = 0;
            plan.steps.push_back(ew);
            written[cur_t] = 1;
        }
        if (op_done[cur_op]) continue;
        op_done[cur_op] = 1;
        const xfr_op_desc& d = e->ops[cur_op].d;
        BwdStep st;
        st.op = cur_op; st.src_t = cur_t;
        auto target = [&](int ti, BwdStep s2) {
            if (ti == 0) return;   // no gradient wrt the image is needed for P[-2]
            s2.dst_t = ti; s2.accumulate = written[ti] ? 1 : 0; written[ti] = 1;
            plan.steps.push_back(s2);
        };
        switch (d.kind) {
            case XFR_OP_CONV:
            case XFR_OP_LINEAR:
                if (d.stride > 1 && d.in0 != 0 && !written[d.in0]) {
                    BwdStep z; z.kind = ST_ZERO; z.dst_t = d.in0; plan.steps.push_back(z); written[d.in0] = 1;
                }
                st.kind = ST_CONV_BWD; target(d.in0, st); break;
            case XFR_OP_MAXPOOL: st.kind = ST_MAXPOOL_BWD; target(d.in0, st); break;
            case XFR_OP_AVGPOOL:
                if (d.kh == 1 && d.stride == 1) { st.kind = ST_COPY; st.copy_elems_per_sb = e->tens[cur_t].C; }    // identity: a gradient copy (often forwarded away)
                else st.kind = ST_AVGPOOL_BWD;
                target(d.in0, st);
                break;
            case XFR_OP_ADD:
            case XFR_OP_G_ADD:
                st.kind = ST_COPY; st.copy_elems_per_sb = e->tens[cur_t].C;
                target(d.in0, st); target(d.in1, st); break;
            case XFR_OP_CONCAT:
                st.kind = ST_COPY; st.copy_elems_per_sb = e->tens[d.in0].C; target(d.in0, st); break;
            case XFR_OP_G_MAXHALVES: {
                // the VJP of max(split[0], split[1]) as the HEAD of an elementwise chain over the 2*Co-channel Split tensor: it then
                // merges with the hook chain that follows (fuse_plan) instead of writing the routed gradient out and reading it back
                st.kind = ST_EW;
                st.ew_t = d.in0;
                BwdStep::Sym sy;
                sy.type = EW_MAXHALF_IN; sy.action = e->tens[d.out].C; sy.t0 = d.in0; sy.x_t = -1; sy.f = 0.f; sy.op = cur_op; sy.slot = -1; sy.tap = false;
                st.chain.push_back(sy);
                target(d.in0, st);
                break;
            }
            case XFR_OP_G_NORMALIZE: st.kind = ST_NORMALIZE_BWD; target(d.in0, st); break;
            default:
                return fail(XFR_UNSUPPORTED_LAYER, "backward: unsupported kind %d", d.kind);
        }
    }
    return fail(XFR_STATE_ERROR, "backward schedule never reached the first layer's output");
}

xfr_status get_plan(xfr_engine* e, int seed_tensor, BwdPlan** out, bool plain)
{
    for (auto& p : e->plans)
        if (p.seed_tensor == seed_tensor && p.mode == e->mode && p.plain == plain) { *out = &p; return XFR_OK; }
    e->plans.emplace_back();
    xfr_status st = make_plan(e, seed_tensor, e->plans.back(), plain);
    if (st != XFR_OK) { e->plans.pop_back(); return st; }
    if (!plain) fuse_plan(e, e->plans.back());
    *out = &e->plans.back();
    return XFR_OK;
}

}  // namespace xfr
