// plan_describe.hip -- the C ABI's window on the planner: everything plan.hip, plan_fuse.hip and the forward fusers decide for a layer program, as text.
// tools/plan_digest.py hashes it over every backbone, mode and fusion level; tools/gen_chain_sigs.py builds chain_sigs.inc from it.
#include "engine_internal.h"

extern "C" {

// Device-free: builds the planner state of an engine (no HIP call, fake base addresses that are never dereferenced) and
// writes the fused schedules as text.
xfr_status xfr_plan_describe(const xfr_op_desc* ops, int32_t n_ops, int32_t n_weights, int32_t in_c, int32_t in_h, int32_t in_w,
                             int32_t batch, int32_t subtree_mode, int32_t seed_tensor, char* buf, size_t capacity, size_t* needed)
{
    if (!ops || n_ops < 2 || in_c < 1 || in_h < 1 || in_w < 1 || batch < 1 || n_weights < 0)
        return fail(XFR_INVALID_ARG, "xfr_plan_describe: bad arguments");
    if (subtree_mode < 0 || subtree_mode > 3) return fail(XFR_INVALID_ARG, "Invalid subtree mode %d", subtree_mode);
    if (ops[0].kind != XFR_OP_CONV || ops[0].in0 != 0)
        return fail(XFR_UNSUPPORTED_LAYER, "the first layer must be a convolution on the input image");
    xfr_engine* e = new xfr_engine();
    struct Del { xfr_engine* e; ~Del() { e->ws.p = nullptr; e->arena.p = nullptr; delete e; } } del{e};      // (the stand-in addresses below are nobody's to free)
    e->max_batch = batch; e->in_c = in_c; e->in_h = in_h; e->in_w = in_w; e->n_weights = n_weights;
    e->mode = subtree_mode;
    e->planning_only = true;
    // tools/gen_chain_sigs.py lists the chains of the test / A-B fusion levels too (XFR_DESCRIBE_FUSION = an xfr_engine_set_epilogue_fusion value)
    if (const char* f = getenv("XFR_DESCRIBE_FUSION")) xfr_engine_set_epilogue_fusion(e, atoi(f));
    xfr_status st = build(e, ops, n_ops);
    if (st == XFR_OK) st = layout_arena(e);
    if (st == XFR_OK) st = layout_workspace(e);
    if (st != XFR_OK) return st;
    if (seed_tensor < 2 || seed_tensor >= (int)e->tens.size()) return fail(XFR_INVALID_ARG, "bad seed tensor %d", seed_tensor);
    e->ws.p = reinterpret_cast<float*>((uintptr_t)1 << 40);
    e->arena.p = reinterpret_cast<float*>((uintptr_t)2 << 40);
    compute_need(e);
    BwdPlan* plan = nullptr;
    st = get_plan(e, seed_tensor, &plan);
    if (st != XFR_OK) return st;
    std::string out;
    char line[512];
    auto emit_sig = [&](const EwChain& ch) {
        uint16_t codes[XFR_MAX_EW_STEPS];
        const int n = ew_chain_codes(ch, codes);
        out += " SIG";
        for (int i = 0; i < n; ++i) { snprintf(line, sizeof(line), " %04x", codes[i]); out += line; }
        snprintf(line, sizeof(line), " compiled=%d", n > 0 ? conv_gemm_chain_sig(ch) : -1);
        out += line;
    };
    snprintf(line, sizeof(line), "plan seed_tensor %d mode %d firings %d launches %zu (unfused %zu)\n", seed_tensor, subtree_mode,
             plan->n_firings, plan->fused_gemm.size(), plan->steps.size());
    out += line;
    // the hooked module call behind every firing, reference order (the image hook of op 0, which the engine does not compute, comes last there)
    out += "firing_ops";
    for (int op : plan->firing_ops) { snprintf(line, sizeof(line), " %d", op); out += line; }
    out += "\n";
    // One convolution of a forward of the given kind: the epilogue its fuser builds, as a SIG line.  Returns 1 if the convolution got one.
    enum FwdKind { FWD_ONLY, FWD_PROBE, FWD_LEAN };
    static const char* fwd_names[] = {"fwd", "probe", "lean-probe"};
    auto fwd_sig = [&](int k, FwdKind kind) -> int {
        const xfr_op_desc& d = e->ops[k].d;
        ConvParams p;
        conv_geometry(e, k, batch, p);
        p.out0 = e->T(d.out);
        if (e->ops[k].groups > 1) {
            // a grouped layer: no epilogue, one launch of the grouped kernel over all groups (per-group Ci, Co and K)
            if (kind == FWD_LEAN) return 0;
            const int G = e->ops[k].groups;
            snprintf(line, sizeof(line), "%s GROUPED op %d [%d x %d x %d] groups %d Ci %d Co %d K %d M %d cfg %d\n", fwd_names[kind], k, e->tens[d.out].C,
                     e->tens[d.out].H, e->tens[d.out].W, G, e->ops[k].Cin / G, d.cout / G, p.K, p.M, CFG_GROUP);
            out += line;
            return 0;
        }
        if (kind == FWD_LEAN) {
            const bool dual = e->tens[d.out].need_pv && e->tens[d.in0].nonneg;
            if (e->ops[k].pair || !dual) return 0;
            fuse_probe_forward(e, k, batch, p, nullptr, dual);
            if (p.chain.n == 0 || p.chain.s[0].type != EW_LEAN_Q) return 0;
        } else {
            if (fuse_mfm_forward(e, k, batch, kind == FWD_PROBE, p)) { }
            else if (kind == FWD_ONLY) fuse_forward_only(e, k, batch, p, nullptr);
            else fuse_probe_forward(e, k, batch, p, nullptr);
            if (p.chain.n == 0) return 0;
        }
        EwLoads ld;
        ew_plan_loads(p.chain, p.out0, ld, EW_FWD_SLOTS_WIDE);
        snprintf(line, sizeof(line), "%s CONV op %d [%d x %d x %d] K %d", fwd_names[kind], k, e->tens[d.out].C, e->tens[d.out].H, e->tens[d.out].W, e->ops[k].K);
        out += line;
        emit_sig(p.chain);
        out += "\n";
        return 1;
    };
    // ... and every convolution up to the seed tensor (a forward-only run skips the ones an earlier epilogue has absorbed).  Returns the lines printed.
    const int last_op = e->tens[seed_tensor].producer;
    e->fwd_last_op = last_op;
    auto fwd_sigs = [&](FwdKind kind) {
        e->fwd_done.assign(e->ops.size(), 0);
        e->pos_done.assign(e->ops.size(), 0);
        int n = 0;
        for (int k = 0; k <= last_op; ++k) {
            const xfr_op_desc& d = e->ops[k].d;
            if ((kind == FWD_ONLY && e->fwd_done[k]) || (d.kind != XFR_OP_CONV && d.kind != XFR_OP_LINEAR)) continue;
            n += fwd_sig(k, kind);
        }
        return n;
    };
    // A schedule, one line per step.  SCHED_FULL: every step with its shape; SCHED_OBSERVED: only the GEMMs that carry a chain; SCHED_LEAN: only the steps
    // that carry a chain.
    enum SchedStyle { SCHED_FULL, SCHED_OBSERVED, SCHED_LEAN };
    const SweepCtx plain;      // the plain sweep: what is described observes nothing
    static const char* kn[] = {"EW", "CONV_BWD", "MAXPOOL_BWD", "AVGPOOL_BWD", "COPY", "MAXHALVES_BWD", "NORMALIZE_BWD", "ZERO"};
    auto print_schedule = [&](const char* prefix, const std::vector<BwdStep>& steps, SchedStyle style) {
        for (const BwdStep& b : steps) {
            if (style != SCHED_FULL && b.chain.empty()) continue;
            if (style == SCHED_OBSERVED && b.kind != ST_CONV_BWD) continue;
            snprintf(line, sizeof(line), "%s %s src %d dst %d", prefix, kn[b.kind], b.src_t, b.dst_t);
            out += line;
            if (style != SCHED_LEAN) { snprintf(line, sizeof(line), " acc %d", b.accumulate); out += line; }
            if (style == SCHED_FULL) {
                const int tt = b.kind == ST_EW ? b.ew_t : b.dst_t;
                if (tt >= 0) { snprintf(line, sizeof(line), " [%d x %d x %d]", e->tens[tt].C, e->tens[tt].H, e->tens[tt].W); out += line; }
                if (b.kind == ST_CONV_BWD) { snprintf(line, sizeof(line), " K %d", e->ops[b.op].Kb); out += line; }
                if (b.kind == ST_CONV_BWD && e->ops[b.op].groups > 1) {      // the backward-data GEMM of a grouped layer: Ci and Co of the GEMM (the layer's swapped)
                    // (M 0: the layer runs by phases, whose PHASE lines below carry their own M)
                    const OpRec& go = e->ops[b.op];
                    ConvParams gp;
                    const bool one = go.phases.empty() && bwd_conv_params(e, plain, *plan, b, batch, 2 * batch, 2 * batch, gp);
                    snprintf(line, sizeof(line), " groups %d Ci %d Co %d M %d cfg %d", go.groups, go.d.cout / go.groups, go.Cin / go.groups, one ? gp.M : 0, CFG_GROUP);
                    out += line;
                }
            }
            if (!b.chain.empty()) {
                EwChain ch;
                EwLoads ld;
                resolve_chain(e, plain, b.chain, ch, nullptr, 2 * batch);
                ew_plan_loads(ch, e->G(b.dst_t), ld, b.kind == ST_CONV_BWD ? EW_FWD_SLOTS_WIDE : EW_FWD_SLOTS_BASE);
                if (b.kind == ST_CONV_BWD) emit_sig(ch);
                else { snprintf(line, sizeof(line), " steps %d", ch.n); out += line; }
                if (style == SCHED_FULL && getenv("XFR_DESCRIBE_TYPES")) {
                    out += " types";
                    for (const auto& y : b.chain) { snprintf(line, sizeof(line), " %d:%d:%d", y.type, y.action, y.t0); out += line; }
                }
            }
            out += "\n";
            // a strided KxK layer: the launches of its phases (two gradient streams of `batch` images), each with the kernel the rules give it
            if (style == SCHED_FULL && b.kind == ST_CONV_BWD)
                for (const PhaseRec& ph : e->ops[b.op].phases) {
                    ConvParams p;
                    if (!bwd_conv_params(e, plain, *plan, b, batch, 2 * batch, 2 * batch, p, &ph)) continue;
                    const int G = e->ops[b.op].groups;
                    snprintf(line, sizeof(line), "%s PHASE op %d (%d,%d) kernel %dx%d cfg %d K %d M %d origin (%d,%d) grid %d x %d", prefix, b.op, ph.r, ph.c,
                             ph.ka, ph.kb, G > 1 ? (int)CFG_GROUP : conv_gemm_pick_cfg(p), p.K, p.M, ph.ih0, ph.iw0, ph.nq, ph.nu);
                    out += line;
                    if (G > 1) { snprintf(line, sizeof(line), " groups %d Ci %d Co %d", G, e->ops[b.op].d.cout / G, e->ops[b.op].Cin / G); out += line; }
                    out += "\n";
                }
        }
    };
    // forward-only runs (encode / the gallery of a triplet step): Conv -> BatchNorm [-> Add] [-> ReLU] epilogues
    fwd_sigs(FWD_ONLY);
    // the probe forward (positive pass alongside): Conv -> BatchNorm [-> ReLU] with the raw output kept
    fwd_sigs(FWD_PROBE);
    print_schedule("bwd", plan->fused_gemm, SCHED_FULL);
    // the schedule of the OBSERVING calls (priors / captures / stored firings: layerwise and weighted-subtree EBP): chains stay in their own launches there,
    // but copy forwarding leaves short hook-free chains (fan-in adds, store-backs) behind some GEMMs -- listed so that they get compiled epilogues too
    print_schedule("observed-bwd", plan->fused, SCHED_OBSERVED);
    // the lean schedule of the same plan (xfr_engine_set_lean): probe-forward epilogues over two accumulator tiles, sweep chains on stored quotients
    lean_prepare(e, *plan, batch);
    if (plan->lean_state == 1) {
        int n_lean = 0;
        { Scoped<const BwdPlan*> lean_cur(e->lean_cur, plan); n_lean = fwd_sigs(FWD_LEAN); }
        print_schedule("lean-bwd", plan->fused_gemm_lean, SCHED_LEAN);
        snprintf(line, sizeof(line), "lean convolutions %d\n", n_lean);
        out += line;
    }
    if (needed) *needed = out.size() + 1;
    if (buf && capacity > 0) {
        const size_t n = std::min(out.size(), capacity - 1);
        memcpy(buf, out.data(), n);
        buf[n] = 0;
    }
    return XFR_OK;
}

}  // extern "C"
