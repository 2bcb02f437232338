// backward.hip -- the sweep executor: resolves a schedule's symbolic chains (plan.hip, plan_fuse.hip) against the workspace and launches it.
#include "engine_internal.h"

namespace xfr {

static int prior_action_for(int mode, int kind)
{   // what the hook returns for a sample whose p was overridden by a prior (whitebox.py:396-428 with p_prior set)
    switch (mode) {
        case XFR_MODE_AFFINEONLY: return is_affine_name(kind) ? PRIOR_DIV : PRIOR_PASS;
        case XFR_MODE_AFFINEONLY_WITH_PRIOR: return is_affine_name(kind) ? PRIOR_DIV : PRIOR_GATEZ;
        case XFR_MODE_NORELU: return (kind == XFR_OP_MAXPOOL || kind == XFR_OP_RELU) ? PRIOR_PASS : PRIOR_DIV;
        default: return PRIOR_DIV;
    }
}

// Symbolic chain -> pointers.  What the fields of the overloaded chain heads and stores mean (EW_POOL2_IN, EW_AVGUP_IN, EW_STORE actions 1 / 2) is
// written down once, at their constructors in plan_fuse.hip (fuse_pool2_head, fuse_avgup_head, fuse_store_save / _restore).
void resolve_chain(xfr_engine* e, const SweepCtx& cx, const std::vector<BwdStep::Sym>& syms, EwChain& ch, double* trace, int SB, bool plain)
{
    ch.n = 0;
    for (const auto& sy : syms) {
        EwStep& q = ch.s[ch.n++];
        memset(&q, 0, sizeof(q));
        q.type = sy.type;
        q.action = sy.action;
        q.f = sy.f;
        q.prior_sb = -1;
        switch (sy.type) {
            case EW_HOOK:
                if (sy.action >= HOOK_Q) {        // lean hooks (lean_rewrite_chain): one source, nothing observed
                    q.p0 = (sy.action == HOOK_Q && sy.x_t >= 0) ? e->Pv(sy.x_t) : e->T(sy.t0);
                    break;
                }
                q.p0 = e->T(sy.t0);
                q.p1 = sy.x_t >= 0 ? e->Pv(sy.x_t) : nullptr;
                if (sy.tap) q.pstore = e->ws + e->tap_off;
                if (e->trace_on && sy.slot >= 0 && trace) q.trace = trace + (size_t)sy.slot * SB;
                if (sy.slot >= 0) {
                    if (sy.slot == cx.store_slot && !sy.tap) q.pstore = cx.store_dst;
                    if (cx.priors && sy.slot == cx.dense_slot) {
                        q.prior_sb = 0;
                        q.prior_dense = cx.prior_dense;
                        q.prior_action = prior_action_for(e->mode, e->ops[sy.op].d.kind);
                    } else if (cx.priors && sy.slot < (int)cx.prior_row.size() && cx.prior_row[sy.slot]) {
                        q.prior_elem = cx.tab_elem + (size_t)sy.slot * cx.tab_sb;
                        q.prior_val = cx.tab_val + (size_t)sy.slot * cx.tab_sb;
                        q.prior_action = prior_action_for(e->mode, e->ops[sy.op].d.kind);
                    }
                    if (cx.caps && sy.slot < (int)cx.cap_row.size() && cx.cap_row[sy.slot]) {
                        q.cap_elem = cx.tab_elem + (size_t)sy.slot * cx.tab_sb;
                        q.cap_dst = cx.cap_dst + (size_t)sy.slot * cx.tab_sb;
                    }
                }
                break;
            case EW_MASK: q.p0 = e->T(sy.t0); break;
            case EW_MAXHALF_IN: q.p0 = e->T(sy.t0); break;
            case EW_POOL2_IN: q.p0 = reinterpret_cast<const float*>(e->idx_base() + e->ops[sy.op].idx_off); break;      // the max-pool's argmax bytes
            case EW_AVGUP_IN:
                // (fuse_avgup_head) sy.action: the pooled tensor's hook (or -1 / -2), sy.t0 / sy.x_t: its a / x tensors (-1: not observed / x == a),
                // sy.op: full-res width, sy.slot: the tensor whose gradient region holds the compact GEMM result (-1: none)
                q.p0 = sy.t0 >= 0 ? e->T(sy.t0) : nullptr;
                q.p1 = sy.x_t >= 0 ? e->Pv(sy.x_t) : nullptr;
                q.p2 = sy.slot >= 0 ? e->G(sy.slot) : nullptr;
                q.prior_sb = sy.op;
                break;
            case EW_MAXHALF_OUT: q.p0 = e->T(sy.t0); break;
            case EW_SCALE_C: q.p0 = e->arena + (plain ? e->ops[sy.op].bn_alpha_t : e->ops[sy.op].bn_alpha_p); break;
            case EW_STORE: q.pstore = sy.t0 >= 0 ? e->G(sy.t0) : nullptr; break;      // action 1 (save) has no destination
            case EW_ADDP: q.p0 = e->G(sy.t0); break;
            default: break;
        }
    }
}

// launch parameters of a backward-data GEMM step (with its fused chain resolved against the workspace); ph: the phase of a strided KxK layer.
// false: a layer that runs by phases was asked for without one, or a phase came with another layer -- p is not a launch
bool bwd_conv_params(xfr_engine* e, const SweepCtx& cx, const BwdPlan& plan, const BwdStep& st, int B, int SB, int SBa, ConvParams& p, const PhaseRec* ph)
{
    const OpRec& o = e->ops[st.op];
    const xfr_op_desc& d = o.d;
    const Tensor& a = e->tens[d.in0];
    const Tensor& t = e->tens[d.out];
    memset(&p, 0, sizeof(p));
    if ((ph != nullptr) != !o.phases.empty() || (st.compact && ph)) return false;
    p.in = e->G(st.src_t);
    if (!ph) p.w = e->arena + (plan.plain ? o.w_bwd_true : o.w_bwd);
    p.out0 = e->G(st.dst_t);
    p.Cin = t.C; p.H = t.H; p.W = t.W; p.NB = SBa; p.in_nb = SB; p.out_nb = SB;
    p.tap_major = (d.stride == 1 && o.tap_bwd && o.groups <= 1) ? 1 : 0;
    p.in_bytes = (unsigned)((size_t)SB * t.per_n() * sizeof(float));
    p.CoutTot = a.C; p.nhalves = 1; p.ldw = o.ldb;
    p.K = o.Kb;
    p.accumulate = st.accumulate;
    if (o.groups > 1) {
        // a grouped layer: the same GEMM per group with the roles of Ci and Co swapped (conv_group.hip) -- no chain, no compact form
        if (st.compact || !st.chain.empty()) return false;
        p.groups = o.groups; p.ldw = GROUP_ROWS;
    }
    if (st.compact) {
        // 1x1 stride-s, result left on the sampled grid (dense rows of t.H x t.W per sample): EW_AVGUP_IN places it
        p.kh = 1; p.kw = 1; p.stride = 1; p.pad = 0;
        p.OH = t.H; p.OW = t.W;
        p.out_H = t.H; p.out_W = t.W; p.out_stride = 1;
        p.accumulate = st.accumulate;           // a second strided GEMM onto the same tensor adds to the first one's rows
        p.as_strided = 1;
    } else if (d.stride == 1) {
        // backward-data of a stride-1 convolution == convolution with the flipped, transposed kernel and padding k-1-p
        p.kh = d.kh; p.kw = d.kw; p.stride = 1; p.pad = d.kh - 1 - d.pad; p.pad_dw = d.kw - d.kh;
        p.OH = a.H; p.OW = a.W;
        p.out_H = a.H; p.out_W = a.W; p.out_stride = 1;
    } else if (ph) {
        // one phase of a strided KxK layer: a stride-1 convolution of dY with the phase's flipped sub-kernel, its nq x nu results scattered
        // with the layer's stride from the phase's first pixel on
        p.w = e->arena + (plan.plain ? ph->w_bwd_true : ph->w_bwd);
        p.K = ph->K;
        p.tap_major = (ph->tap && o.groups <= 1) ? 1 : 0;
        p.kh = ph->ka; p.kw = ph->kb; p.stride = 1; p.pad = ph->ka - 1 - ph->q0; p.pad_dw = (ph->kb - 1 - ph->u0) - p.pad;
        p.OH = ph->nq; p.OW = ph->nu;
        p.out0 = e->G(st.dst_t) + (size_t)ph->ih0 * a.W + ph->iw0;
        p.out_H = a.H; p.out_W = a.W; p.out_stride = d.stride;
        p.accumulate = 1;   // the target was zero-filled or already holds other contributions
    } else {
        // 1x1 stride-s: the gradient lands on the sampled grid only
        p.kh = 1; p.kw = 1; p.stride = 1; p.pad = 0;
        p.OH = t.H; p.OW = t.W;
        p.out_H = a.H; p.out_W = a.W; p.out_stride = d.stride;
        p.accumulate = 1;   // the target was zero-filled or already holds other contributions
    }
    p.M = SBa * p.OH * p.OW;
    if (!st.chain.empty()) {
        resolve_chain(e, cx, st.chain, p.chain, nullptr, SB);
        p.chain_B = B;
        p.chain_eps = e->eps;
        p.accumulate = 0;
        if (e->pair_tiles && SBa == 2 * B) p.pair_m = B * p.OH * p.OW;     // the two streams' tiles of one position side by side (ConvParams::pair_m)
    }
    p.chain_interpret = e->interpret_chains ? 1 : 0;
    p.bwd = 1;
    return true;
}

// The fan-out schedule (plan.fused_gemm: MaxFeatureMap VJPs inside GEMM epilogues) only runs where every such epilogue is COMPILED --
// the interpreter has no fan-out step.  Every other fusion falls back to the interpreted epilogue; a network whose merged fan-out
// chain is not in chain_sigs.inc falls back to the schedule without fan-outs (plan.fused_gemm_nofan).  Decided once per plan: whether
// a chain has a compiled signature depends on the layer program and the mode, not on the batch (the fan-out requires HW % 4 == 0).
static bool fanout_compiled(xfr_engine* e, const SweepCtx& cx, BwdPlan& plan, int B, int SB)
{
    if (plan.fan_ok >= 0) return plan.fan_ok != 0;
    plan.fan_ok = 1;
    for (const BwdStep& st : plan.fused_gemm) {
        if (st.kind != ST_CONV_BWD) continue;
        bool fan = false;
        for (const auto& sy : st.chain) if (sy.type == EW_MAXHALF_OUT) fan = true;
        if (!fan) continue;
        ConvParams p;
        if (!bwd_conv_params(e, cx, plan, st, B, SB, SB, p)) { plan.fan_ok = 0; break; }      // (a layer that runs by phases carries no chain)
        p.chain_interpret = 0;
        if (conv_gemm_cannot_launch(p)) { plan.fan_ok = 0; break; }
    }
    return plan.fan_ok != 0;
}

xfr_status run_backward(xfr_engine* e, const SweepCtx& cx, BwdPlan& plan, int B, int S, hipStream_t s)
{
    const int SB = S * B;
    double* trace = e->dbl_ws + 2 * e->max_batch;
    if (e->trace_on) {
        HIP_TRY(hipMemsetAsync(trace, 0, sizeof(double) * (size_t)plan.n_firings * SB, s));
        e->last_trace_firings = plan.n_firings;
        e->last_trace_sb = SB;
        e->last_trace_kinds = plan.firing_kinds;
    }
    const bool special = cx.observing();
    const bool use_fused = !e->trace_on && !plan.fused.empty() && !plan.plain;
    // Layerwise sweeps sorted by firing (cx.active): stream j is identically zero until the step that holds its prior
    // hook, so the GEMMs and hook chains before that step leave it out (the gradient region was zero-filled; the small
    // pool / copy kernels still run over all streams and move zeros).  SBa = streams alive at this step.
    const bool prefix = !cx.active.empty() && (int)cx.active.size() * cx.n == SB;
    int run_max = -1;
    const bool use_gemm_fusion = use_fused && e->fuse_gemm_epilogue && !special && !plan.fused_gemm.empty();
    const bool fanout = use_gemm_fusion && !e->interpret_chains && fanout_compiled(e, cx, plan, B, SB);
    const bool lean = e->lean_cur == &plan && use_gemm_fusion && plan.lean_state == 1;
    if (e->lean_cur == &plan && !lean) return fail(XFR_STATE_ERROR, "lean schedule: the probe forward ran lean and the sweep cannot");
    // On-demand zeroing of the prefix sweeps (cx.lazy_zero): wr[t] = leading rows of G(t) that hold defined values.  A launch that reads rows
    // [0, r) first gets the rows [wr[t], r) zeroed (one 2-D memset over the channels); launches that walk whole tensors or use another layout
    // (pool / copy VJPs, scattering and compact strided GEMMs, chain heads that expand a pooled gradient) get whole tensors.
    const bool lazy = prefix && cx.lazy_zero;
    std::vector<int> wr;
    if (lazy) { wr.assign(e->tens.size(), 0); wr[plan.seed_tensor] = SB; }
    auto need = [&](int t, int rows) -> xfr_status {
        if (!lazy || t < 0 || wr[t] >= rows) return XFR_OK;
        const Tensor& x = e->tens[t];
        const size_t hw = (size_t)x.HW();
        HIP_TRY(hipMemset2DAsync(e->G(t) + (size_t)wr[t] * hw, (size_t)SB * hw * sizeof(float), 0, (size_t)(rows - wr[t]) * hw * sizeof(float), (size_t)x.C, s));
        wr[t] = rows;
        return XFR_OK;
    };
    auto wrote = [&](int t, int rows) { if (lazy && t >= 0 && wr[t] < rows) wr[t] = rows; };
    for (const BwdStep& st : (lean ? plan.fused_gemm_lean : use_gemm_fusion ? (fanout ? plan.fused_gemm : plan.fused_gemm_nofan) : use_fused ? plan.fused : plan.steps)) {
        int SBa = SB;
        if (prefix) {
            for (const auto& sy : st.chain)
                if (sy.type == EW_HOOK && sy.slot > run_max) run_max = sy.slot;
            SBa = (int)(std::upper_bound(cx.active.begin(), cx.active.end(), run_max) - cx.active.begin()) * cx.n;
            if (SBa == 0) continue;
        }
        if (lazy) {
            bool irregular = st.compact || !(st.kind == ST_EW || st.kind == ST_CONV_BWD);
            if (st.kind == ST_CONV_BWD && e->ops[st.op].d.stride != 1) irregular = true;
            for (const auto& sy : st.chain)
                if (sy.type == EW_AVGUP_IN || sy.type == EW_POOL2_IN || sy.type == EW_MAXHALF_IN || sy.type == EW_MAXHALF_OUT) irregular = true;
            const int ew_hw = st.kind == ST_EW ? e->tens[st.ew_t].HW() : 4;
            // rows this launch covers: the float4 chain kernel and the GEMMs honour the prefix, the scalar chain kernels walk every row
            const int rows = (irregular || st.kind == ST_ZERO || (st.kind == ST_EW && ((ew_hw & 3) != 0 || st.accumulate))) ? SB : SBa;
            xfr_status zs = XFR_OK;
            if (st.kind != ST_ZERO && zs == XFR_OK) zs = need(st.src_t, rows);
            if ((st.accumulate || irregular) && zs == XFR_OK) zs = need(st.dst_t, rows);
            for (const auto& sy : st.chain) {
                if (zs != XFR_OK) break;
                if (sy.type == EW_ADDP) zs = need(sy.t0, rows);
                else if (sy.type == EW_AVGUP_IN && sy.slot >= 0) zs = need(sy.slot, SB);
            }
            if (zs != XFR_OK) return zs;
            wrote(st.dst_t, rows);
            for (const auto& sy : st.chain)
                if (sy.type == EW_STORE && sy.action != 1) wrote(sy.t0, rows);
        }
        switch (st.kind) {
            case ST_EW: {
                EwChain ch;
                resolve_chain(e, cx, st.chain, ch, trace, SB, plan.plain);
                const Tensor& x = e->tens[st.ew_t];
                launch_ew_chain(e->G(st.src_t), e->G(st.dst_t), st.accumulate, ch, x.C, SB, B, x.HW(), e->eps, s, SBa);
                break;
            }
            case ST_ZERO:
                launch_fill(e->G(st.dst_t), (long)SB * e->tens[st.dst_t].per_n(), 0.f, s);
                break;
            case ST_CONV_BWD: {
                ConvParams p;
                const std::vector<PhaseRec>& phases = e->ops[st.op].phases;
                if (!phases.empty() && !st.chain.empty()) return fail(XFR_STATE_ERROR, "a scattering backward-data GEMM cannot carry a fused chain");
                // A strided KxK layer: one launch per phase, each onto its own pixels of the (zero-filled) target.  The phases write disjoint pixels and
                // read the same gradient, so they run side by side: phase q on the sweep's stream (q % 4 == 0) or on a side stream, forked behind what
                // the sweep has enqueued and joined before its next step.  Same launches, same bits.  A profiled run times launches one by one: in a row.
                PhaseStreams* side = nullptr;
                if (phases.size() > 1 && e->overlap_phases && !e->profile_on) {
                    if (!e->ph_streams) {
                        std::unique_ptr<PhaseStreams> g(new PhaseStreams());
                        XFR_TRY(g->fork.create());
                        for (int i = 0; i < 3; ++i) { XFR_TRY(g->s[i].create()); XFR_TRY(g->done[i].create()); }
                        e->ph_streams = std::move(g);
                    }
                    side = e->ph_streams.get();
                    HIP_TRY(hipEventRecord(side->fork, s));
                    for (int i = 0; i < 3 && i + 1 < (int)phases.size(); ++i) HIP_TRY(hipStreamWaitEvent(side->s[i], side->fork, 0));
                }
                xfr_status rs = XFR_OK;
                for (size_t q = 0; q < std::max<size_t>(phases.size(), 1) && rs == XFR_OK; ++q) {
                    if (!bwd_conv_params(e, cx, plan, st, B, SB, SBa, p, phases.empty() ? nullptr : &phases[q]))
                        rs = fail(XFR_STATE_ERROR, "backward-data GEMM of op %d: phase and layer do not match", st.op);
                    else
                        rs = run_conv(e, p, (side && (q & 3)) ? (hipStream_t)side->s[(q & 3) - 1] : s);
                }
                if (side)      // the join, on every way out: the sweep goes on behind whatever the side streams hold
                    for (int i = 0; i < 3 && i + 1 < (int)phases.size(); ++i) {
                        HIP_TRY(hipEventRecord(side->done[i], side->s[i]));
                        HIP_TRY(hipStreamWaitEvent(s, side->done[i], 0));
                    }
                if (rs != XFR_OK) return rs;
                break;
            }
            case ST_MAXPOOL_BWD: {
                const OpRec& o = e->ops[st.op];
                const xfr_op_desc& d = o.d;
                const Tensor& a = e->tens[d.in0];
                const Tensor& t = e->tens[d.out];
                launch_maxpool_bwd(e->G(st.src_t), e->idx_base() + o.idx_off, e->G(st.dst_t), st.accumulate, a.C, SB, B, a.H, a.W, t.H,
                                   t.W, d.kh, d.stride, d.pad, s);
                break;
            }
            case ST_AVGPOOL_BWD: {
                const xfr_op_desc& d = e->ops[st.op].d;
                const Tensor& a = e->tens[d.in0];
                const Tensor& t = e->tens[d.out];
                launch_avgpool_bwd(e->G(st.src_t), e->G(st.dst_t), st.accumulate, a.C * SB, a.H, a.W, t.H, t.W, d.kh, d.stride, s);
                break;
            }
            case ST_COPY: {
                const Tensor& dt = e->tens[st.dst_t];
                launch_copy_acc(e->G(st.src_t), e->G(st.dst_t), (long)st.copy_elems_per_sb * SB * dt.HW(), st.accumulate, s);
                break;
            }
            case ST_MAXHALVES_BWD: {
                const xfr_op_desc& d = e->ops[st.op].d;
                const Tensor& t = e->tens[d.out];
                launch_maxhalves_bwd(e->G(st.src_t), e->T(d.in0), e->G(st.dst_t), st.accumulate, t.C, SB, B, t.HW(), s);
                break;
            }
            case ST_NORMALIZE_BWD: {
                const OpRec& o = e->ops[st.op];
                const xfr_op_desc& d = o.d;
                const Tensor& t = e->tens[d.out];
                launch_normalize_bwd(e->G(st.src_t), e->T(d.in0), e->misc() + o.norm_off, e->G(st.dst_t), st.accumulate,
                                     t.C, SB, B, s);
                break;
            }
        }
    }
    return XFR_OK;
}

}  // namespace xfr
