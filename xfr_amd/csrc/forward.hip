// forward.hip -- the forward executor: true values and, for a probe, the positive pass, with the elementwise ops behind a convolution folded into its
// GEMM epilogue where a fuser finds them.  The fusers decide and build pointers in one go (and launch a hoisted shortcut through operand_ready).
#include "engine_internal.h"

namespace xfr {
namespace {

// x source of a hook / positive-pass value of a tensor, as (pointer, relu-on-load)
struct Src { const float* p; int relu; };

Src pv_src(xfr_engine* e, int t)
{
    const Tensor& x = e->tens[t];
    if (x.pstate == PS_EQ) return {e->T(t), 0};
    if (x.pstate == PS_RELU) return {e->T(t), 1};
    return {e->Pv(t), 0};
}

// the next step of a chain under construction, zeroed
EwStep& push(EwChain& ch, int type)
{
    EwStep& q = ch.s[ch.n++];
    memset(&q, 0, sizeof(q));
    q.type = type;
    q.prior_sb = -1;
    return q;
}

}  // namespace

static xfr_status fwd_op(xfr_engine* e, int k, int B, bool want_pos, hipStream_t s, bool keep_raw = false);
static xfr_status pos_op(xfr_engine* e, int k, int B, hipStream_t s);

// ---------------------------------------------------------------------------------------------------------------
// the event pair (and record slot) the next profiled launch takes; it counts as used once that launch is recorded
static xfr_status next_event_pair(xfr_engine* e, std::pair<Event, Event>*& ev)
{
    if (e->ev_used == e->ev_pool.size()) {
        Event a, b;
        XFR_TRY(a.create(true));
        XFR_TRY(b.create(true));
        e->ev_pool.emplace_back(std::move(a), std::move(b));
    }
    if (e->ev_params.size() < e->ev_pool.size()) { e->ev_params.resize(e->ev_pool.size()); e->ev_cfg.resize(e->ev_pool.size()); }
    ev = &e->ev_pool[e->ev_used];
    return XFR_OK;
}

xfr_status run_conv(xfr_engine* e, const ConvParams& p_in, hipStream_t s)
{
    // a grouped layer (conv_group.hip, configuration 13; a depthwise launch: conv_depthwise.hip, configuration 14): no chain, no bf16x6, no tail balancing
    const bool grouped = p_in.groups > 1;
    ConvParams p = p_in;
    p.chain_interpret = e->interpret_chains ? 1 : 0;      // (these three: read by the dense kernels only)
    p.split_ok = (e->split_mask & (p.bwd ? 2 : 1)) ? (e->split_any_grid ? 2 : 1) : 0;
    p.tail_force = e->tail_balance ? 0 : 1;
    if (!grouped && e->tail_balance) {
        int k = 0;
        while (k < e->n_tail_ws && e->tail_ws[k].s != s) ++k;
        if (k == e->n_tail_ws && k < 8) {
            DevBuf<float> ws;      // the workspace, then the tiles' arrival counters
            XFR_TRY(ws.alloc((XFR_TAIL_WS_BYTES + XFR_TAIL_MAX_TILES * sizeof(unsigned)) / sizeof(float)));
            unsigned* cnt = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(ws.p) + XFR_TAIL_WS_BYTES);
            HIP_TRY(hipMemset(cnt, 0, XFR_TAIL_MAX_TILES * sizeof(unsigned)));
            HIP_TRY(hipDeviceSynchronize());
            e->tail_ws[k].s = s; e->tail_ws[k].ws = std::move(ws); e->tail_ws[k].cnt = cnt;
            e->n_tail_ws = k + 1;
        }
        if (k < e->n_tail_ws) {
            p.tail_ws = e->tail_ws[k].ws;
            p.tail_cnt = e->tail_ws[k].cnt;
            p.tail_ws_bytes = XFR_TAIL_WS_BYTES;
        }
    }
    std::pair<Event, Event>* ev = nullptr;
    if (e->profile_on) {
        if (const int why = grouped ? 0 : conv_gemm_cannot_launch(p)) return fail(XFR_STATE_ERROR, "%s", conv_gemm_refusal(why));          // nothing launched: no event pair, no record
        // (HIP events misread the FIRST GEMM of a profiled run -- 0.87 ms for a 0.37 ms stem in round 3, 1.03 ms with a stream synchronise in
        // front of it in round 4: the start event is stamped on a queue that has just been idle.  The per-shape tables of profiles/ therefore
        // also come from the kernels' own stamps: bench.py --serial --launch-log-csv, profiles/layer_table.py.)
        XFR_TRY(next_event_pair(e, ev));
        HIP_TRY(hipEventRecord(ev->first, s));
    }
    int cfg;
    if (grouped) {
        cfg = (e->depthwise_valu && launch_conv_depthwise(p, s)) ? CFG_DEPTHWISE : CFG_GROUP;
        if (cfg == CFG_GROUP && !launch_conv_group(p, s)) return fail(XFR_STATE_ERROR, "a grouped convolution launch (groups %d) the grouped kernel does not take", p.groups);
    } else if (launch_conv_gemm(p, s)) {
        cfg = conv_gemm_last_cfg();
    } else {
        return fail(XFR_STATE_ERROR, "%s", conv_gemm_refusal(conv_gemm_cannot_launch(p)));
    }
    if (ev) {
        e->ev_params[e->ev_used] = p;
        e->ev_cfg[e->ev_used++] = cfg;          // the configuration that ran
        HIP_TRY(hipEventRecord(ev->second, s));
        // (a grouped launch has no dualacc, and its K_logical is its K, the K of ONE group -- conv_geometry: Kf == K, plan.hip -- or 0: bwd_conv_params)
        e->prof_flops += 2.0 * (double)(p.K_logical ? p.K_logical : p.K) * (double)p.M * (double)p.CoutTot * (double)(p.dualacc ? 2 : p.nhalves);
    }
    return XFR_OK;
}

void conv_geometry(xfr_engine* e, int k, int NB, ConvParams& p)
{
    const OpRec& o = e->ops[k];
    const xfr_op_desc& d = o.d;
    const Tensor& a = e->tens[d.in0];
    const Tensor& t = e->tens[d.out];
    memset(&p, 0, sizeof(p));
    p.Cin = a.C; p.H = a.H; p.W = a.W; p.NB = NB;
    p.kh = d.kh; p.kw = d.kw; p.stride = d.stride; p.pad = d.pad;
    p.OH = t.H; p.OW = t.W;
    p.K = o.Kf; p.K_logical = o.K; p.M = NB * t.H * t.W;
    p.ldw = o.ldw;
    p.out_H = t.H; p.out_W = t.W; p.out_stride = 1;
    p.in_nb = NB; p.out_nb = NB;
    p.in_bytes = (unsigned)((size_t)NB * a.per_n() * sizeof(float));
    p.tap_major = o.tap4_fwd ? 2 : (o.tap_fwd ? 1 : 0);
    p.co_pair = o.pair;
    if (o.groups > 1) { p.groups = o.groups; p.tap_major = 0; p.ldw = GROUP_ROWS; }
}

// The reference evaluates a down-sampling block's shortcut BEHIND the main path (resnet.py:144-146: `residual = self.downsample(x)` after
// bn3), so in program order the residual operand does not exist yet when the block's last convolution is launched and the add kept its own
// kernel.  Nothing orders the two branches: when the operand is the end of a short chain of pooling / padding ops over tensors that exist,
// run that chain now (true values and, in a probe forward, its positive values) and mark it done.  Returns true when tensor `t` exists afterwards.
static bool operand_ready(xfr_engine* e, int t, int k, int B, bool with_pos, hipStream_t s)
{
    if (e->tens[t].producer < k) return true;
    if (!e->hoist_shortcut) return false;
    int chain[4], n = 0;
    for (int u = t; e->tens[u].producer >= k; u = e->ops[e->tens[u].producer].d.in0) {
        const int kp = e->tens[u].producer;
        if (e->fwd_done[kp]) break;                       // enqueued already (stream order makes it exist)
        const xfr_op_desc& d = e->ops[kp].d;
        if (kp > e->fwd_last_op || n == 4 || (d.kind != XFR_OP_AVGPOOL && d.kind != XFR_OP_CONCAT)) return false;
        if (with_pos && e->tens[d.out].need_pv && d.kind != XFR_OP_AVGPOOL) return false;     // pos_op computes no padded positive value
        chain[n++] = kp;
    }
    for (int i = n - 1; i >= 0; --i) {
        const int kp = chain[i];
        if (!e->planning_only && !e->dry_run) {
            if (!e->fwd_done[kp] && fwd_op(e, kp, B, with_pos, s) != XFR_OK) return false;
            if (with_pos && e->tens[e->ops[kp].d.out].need_pv && !e->pos_done[kp] && pos_op(e, kp, B, s) != XFR_OK) return false;
        }
        e->fwd_done[kp] = 1;
        e->pos_done[kp] = 1;
    }
    return true;
}

// Forward-only runs (encode, embeddings, the gallery of a triplet step) never need the raw convolution output:
// Conv -> BatchNorm [-> Add with an already computed operand] [-> in-place ReLU] runs in the GEMM's chain epilogue
// (per-channel affine, residual read as 16-byte pieces, clamp), same arithmetic in the same order as the stand-alone
// kernels.
void fuse_forward_only(xfr_engine* e, int k, int B, ConvParams& p, hipStream_t s)
{
    const xfr_op_desc& d = e->ops[k].d;
    const Tensor& c = e->tens[d.out];
    if (c.consumers.size() != 1) return;
    const int k1 = c.consumers[0];
    if (k1 > e->fwd_last_op) return;
    const OpRec& bn = e->ops[k1];
    if (bn.d.kind != XFR_OP_BATCHNORM) return;
    const int bn_out = bn.d.out;
    EwChain& ch = p.chain;
    ch.n = 0;
    {
        EwStep& q = push(ch, EW_AFFINE_C);
        q.p0 = e->arena + bn.bn_alpha_t;
        q.p1 = e->arena + bn.bn_beta_t;
    }
    int final_t = bn_out, k2 = -1;
    bool fused_add = false;
    if (!bn.fuse_relu && e->tens[bn_out].consumers.size() == 1) {
        k2 = e->tens[bn_out].consumers[0];
        const OpRec& ad = e->ops[k2];
        if (k2 <= e->fwd_last_op && (ad.d.kind == XFR_OP_ADD || ad.d.kind == XFR_OP_G_ADD)) {
            const int other = (ad.d.in0 == bn_out) ? ad.d.in1 : ad.d.in0;
            if (other != bn_out && operand_ready(e, other, k, B, false, s)) {          // the other operand is already computed (or is now)
                push(ch, EW_ADDP).p0 = e->T(other);
                if (ad.fuse_relu) push(ch, EW_RELU);
                final_t = ad.d.out;
                fused_add = true;
            }
        }
    }
    if (!fused_add && bn.fuse_relu) push(ch, EW_RELU);
    p.out0 = e->T(final_t);
    p.chain_B = B;
    p.chain_eps = e->eps;
    e->fwd_done[k1] = 1;
    if (fused_add) e->fwd_done[k2] = 1;
}

// The probe forward (with the positive pass) needs more than the gallery forward: the RAW convolution output stays (the
// BatchNorm hook's a is relu(conv output)), and in the modes that divide by a ReLU / Add input's X the BatchNorm's positive
// output is needed too.  Conv -> BatchNorm [-> in-place ReLU] then runs as: STORE raw, [FORK positive BatchNorm], affine, [clamp].
// The residual add is left to its own kernel (its pre-add operand is hook state as well).  Returns false if nothing was fused.
static bool can_fuse_probe(xfr_engine* e, int k, int* k1_out)
{
    const xfr_op_desc& d = e->ops[k].d;
    const Tensor& c = e->tens[d.out];
    if (c.consumers.size() != 1) return false;
    const int k1 = c.consumers[0];
    if (k1 > e->fwd_last_op || e->ops[k1].d.kind != XFR_OP_BATCHNORM) return false;
    *k1_out = k1;
    return true;
}

// Lean variant (`dual` launches of a lean call, xfr_engine_set_lean): the W and relu(W) accumulators meet in ONE workgroup (ConvParams::dualacc), so
// the BatchNorm hook's a / (x + eps) is formed there and stored in place of the raw output (EW_LEAN_Q ... EW_LEAN_STORE); where the in-place ReLU
// behind the BatchNorm [+ functional add] has a dividing hook too, its quotient replaces the positive BatchNorm output (EW_LEAN_XR).  Two
// tensors written per convolution instead of three or four, and the sweep reads one or two instead of three or four.
void fuse_probe_forward(xfr_engine* e, int k, int B, ConvParams& p, hipStream_t s, bool dual, bool lean_try)
{
    int k1 = -1;
    if (!can_fuse_probe(e, k, &k1)) return;
    const xfr_op_desc& d = e->ops[k].d;
    const OpRec& bn = e->ops[k1];
    const int bn_out = bn.d.out;
    EwChain& ch = p.chain;
    ch.n = 0;
    // lean: every hook on the raw output is the BatchNorm's (its a and x are the two accumulators), and the call asked for it
    // (tuning: XFR_LEAN_MAX_K -- only convolutions with at most that many K rows go lean)
    const int lean_max_k = [] { const char* v = getenv("XFR_LEAN_MAX_K"); return v ? atoi(v) : 512; }();
    // ... and for KxK convolutions: their two-accumulator form ties with the dual launch up to K = 1152 (measured, profiles/r5/experiments/lean_k_threshold.txt)
    const int lean_max_k3 = [&] { const char* v = getenv("XFR_LEAN_MAX_K3"); return v ? atoi(v) : std::max(lean_max_k, 1152); }();
    // ... and only where the GEMM has a two-accumulator instantiation: not on the generic (ci, kh, kw) gather, which a KxK layer with Cin % 16 != 0
    // and a strided 1x1 layer with Cin % 16 != 0 take (launch_cfg) -- such a launch was refused and the whole call failed
    const int cin = e->tens[d.in0].C;
    const bool dual_gather = d.kh * d.kw > 1 ? e->ops[k].tap_fwd : ((cin % 16) == 0 || (d.stride == 1 && d.pad == 0));
    bool lean = lean_try && dual && dual_gather && d.out != 1 && e->ops[k].Kf <= (d.kh * d.kw > 1 ? lean_max_k3 : lean_max_k) && e->tens[d.out].need_pv &&
                (e->lean_decide || (e->lean_cur && e->lean_cur->lean_q[d.out] == 1));
    if (lean)
        for (const Hook& h : e->tens[d.out].hooks)
            if (h.op != k1 || h.a_tensor != d.out) lean = false;
    if (lean) push(ch, EW_LEAN_Q);
    else push(ch, EW_STORE).pstore = e->T(d.out);
    int fork_at = -1;
    if (e->tens[bn_out].need_pv) {
        fork_at = ch.n;
        EwStep& q = push(ch, EW_FORK_POSBN);
        q.p0 = e->arena + bn.bn_alpha_p;
        q.p1 = e->arena + (e->with_bias ? bn.bn_beta_pb : bn.bn_beta_p);
        q.pstore = e->Pv(bn_out);
        e->pos_done[k1] = 1;
    }
    {
        EwStep& q = push(ch, EW_AFFINE_C);
        q.p0 = e->arena + bn.bn_alpha_t;
        q.p1 = e->arena + bn.bn_beta_t;
    }
    // The residual add behind the BatchNorm joins the chain where the pre-add tensor is nobody's business afterwards: no hook takes its
    // (a, x) from it (the reference's Add hooks both use the LAST input, the residual: whitebox.py:379-381), and the positive pass
    // does not need the sum's inputs (modes that divide by a ReLU input's X compute it from them: then the add keeps its kernel).
    int final_t = bn_out, k2 = -1, pos_add = -1;
    bool fused_add = false;
    if (!bn.fuse_relu && e->tens[bn_out].consumers.size() == 1 && !e->is_hook_a[bn_out]) {
        k2 = e->tens[bn_out].consumers[0];
        const OpRec& ad = e->ops[k2];
        // (the positive pass of a functional add reads its inputs' POSITIVE values, never the true ones: only the Add module's does)
        if (k2 <= e->fwd_last_op && (ad.d.kind == XFR_OP_G_ADD || (ad.d.kind == XFR_OP_ADD && !e->tens[ad.d.out].need_pv))) {
            const int other = (ad.d.in0 == bn_out) ? ad.d.in1 : ad.d.in0;
            if (other != bn_out && operand_ready(e, other, k, B, true, s)) {
                push(ch, EW_ADDP).p0 = e->T(other);
                if (ad.fuse_relu) push(ch, EW_RELU);
                final_t = ad.d.out;
                fused_add = true;
                // The FUNCTIONAL add's positive-pass output (resnet50_128.py: torch.add(shortcut, 1, bn); 'norelu' / 'all' divide by it at the ReLU
                // behind it) is pv(shortcut) + positive BatchNorm: the fork adds the other operand -- already computed -- and stores the SUM; the
                // BatchNorm's own positive output has no other reader (single consumer, no hook takes its x from it).  One add2 launch per block less.
                if (e->fuse_pools && fork_at >= 0 && ad.d.kind == XFR_OP_G_ADD && e->tens[ad.d.out].need_pv) {
                    const Src o2 = pv_src(e, other);
                    EwStep& q = ch.s[fork_at];
                    q.p2 = o2.p;
                    q.action = o2.relu ? 1 : 0;
                    q.pstore = e->Pv(ad.d.out);
                    pos_add = k2;
                }
            }
        }
    }
    if (!fused_add && bn.fuse_relu) push(ch, EW_RELU);
    int lean_tq = -1;
    if (lean) {
        const bool ends_relu = fused_add ? e->ops[k2].fuse_relu : bn.fuse_relu;
        // the ReLU hook's quotient: the fork's value has one reader, the x of the hook of the in-place ReLU that ends this chain
        if (fork_at >= 0 && ends_relu) {
            const int cand = pos_add >= 0 ? e->ops[pos_add].d.out : (fused_add ? -1 : bn_out);
            if (cand >= 0 && e->tens[cand].consumers.size() == 1 && e->ops[e->tens[cand].consumers[0]].d.kind == XFR_OP_RELU &&
                e->ops[e->tens[cand].consumers[0]].relu_fused_away && e->root(e->ops[e->tens[cand].consumers[0]].d.out) == e->root(final_t))
                lean_tq = cand;
        }
        if (lean_tq >= 0) { ch.s[fork_at].type = EW_LEAN_XR; ch.s[fork_at].pstore = nullptr; }
        { EwStep& q = push(ch, EW_LEAN_STORE); q.action = 0; q.pstore = e->T(d.out); }
        if (lean_tq >= 0) { EwStep& q = push(ch, EW_LEAN_STORE); q.action = 1; q.pstore = e->Pv(lean_tq); }
        if (e->lean_decide) {
            e->lean_q_run[d.out] = 1;
            e->lean_final_run[d.out] = ends_relu ? e->root(final_t) : -1;
            if (lean_tq >= 0) e->lean_q_run[lean_tq] = 2;
        }
    }
    // a dual launch can only carry a chain through the compiled float4 epilogue (conv_gemm.hip): rows that are a multiple of 4
    // long and a signature that is in the table; otherwise the BatchNorm keeps its own kernel
    {
        const Tensor& t = e->tens[d.out];
        EwChain probe = ch;
        EwLoads ld;
        ew_plan_loads(probe, e->T(final_t), ld, EW_FWD_SLOTS_WIDE);
        if (!e->planning_only && ((((long)B * t.HW()) & 3) != 0 || conv_gemm_chain_sig(probe) < 0)) {
            ch.n = 0;
            e->pos_done[k1] = 0;
            if (pos_add >= 0) e->pos_done[pos_add] = 0;
            if (lean) {     // no compiled lean epilogue: the plan as a whole stays literal (lean_prepare), this launch too
                e->lean_missing_sig = true;
                if (e->lean_decide) { e->lean_q_run[d.out] = 0; e->lean_final_run[d.out] = -1; if (lean_tq >= 0) e->lean_q_run[lean_tq] = 0; }
                fuse_probe_forward(e, k, B, p, s, dual, false);
            }
            return;
        }
    }
    p.out0 = e->T(final_t);
    p.chain_B = B;
    p.chain_eps = e->eps;
    e->fwd_done[k1] = 1;
    if (fused_add) e->fwd_done[k2] = 1;
    if (pos_add >= 0) e->pos_done[pos_add] = 1;
}

// MaxFeatureMap in the convolution's epilogue (lightcnn.py:48-62: Conv -> Split -> torch.max of the halves).  The forward pack holds
// the two halves interleaved, so a channel and its partner are neighbouring rows of one accumulator tile: the epilogue stores the raw
// rows where the Split hook and the VJP expect them (keep_raw; a forward-only run needs neither) and the even rows store the maximum.
// Returns false -- nothing fused, the three ops run as before -- where the float4 epilogue does not apply.
bool fuse_mfm_forward(xfr_engine* e, int k, int B, bool keep_raw, ConvParams& p, bool want_pos)
{
    const OpRec& o = e->ops[k];
    if (!o.pair || o.pair_max > e->fwd_last_op || e->interpret_chains) return false;      // the interpreter has no EW_MAXPAIR
    const Tensor& t = e->tens[o.d.out];
    EwChain ch;
    ch.n = 0;
    if (keep_raw) push(ch, EW_STORE).pstore = e->T(o.d.out);
    push(ch, EW_MAXPAIR);
    float* dst = e->T(e->ops[o.pair_max].d.out);
    // The resblock's Add (lightcnn.py:88: out = mfm(mfm(x)) + x) behind the pair maximum: nobody else reads the maximum (the Add hooks take their
    // (a, x) from the LAST input, the residual), so the even rows store the sum -- and, where a hook divides by it, the Add's positive-pass output
    // relu(max) + relu(residual) -- instead of the maximum; the add2 launches (true and positive) go away.
    int k3 = -1;
    {
        const int tmax = e->ops[o.pair_max].d.out;
        const Tensor& tm = e->tens[tmax];
        if (e->fuse_pools && tm.consumers.size() == 1 && !e->is_hook_a[tmax] && !tm.need_pv) {
            const int kc = tm.consumers[0];
            const OpRec& ad = e->ops[kc];
            const int other = ad.d.in0 == tmax ? ad.d.in1 : ad.d.in0;
            if (kc <= e->fwd_last_op && ad.d.kind == XFR_OP_ADD && !ad.fuse_relu && other != tmax && e->tens[other].producer < k &&
                e->tens[other].alias < 0) {
                if (keep_raw && want_pos && e->tens[ad.d.out].need_pv) {      // (raw rows without a positive pass: the weights pass, no positive Add output)
                    EwStep& q = push(ch, EW_FORK_POSADD);
                    q.p0 = e->T(other);
                    q.pstore = e->Pv(ad.d.out);
                    // pos_op: relu on an input unless it is provably >= 0; bit 0 = the maximum, bit 1 = the residual
                    q.action = (tm.nonneg ? 0 : 1) | (e->tens[other].nonneg ? 0 : 2);
                }
                push(ch, EW_ADDP_CO).p0 = e->T(other);
                dst = e->T(ad.d.out);
                k3 = kc;
            }
        }
    }
    if (!e->planning_only) {
        if ((((long)B * t.HW()) & 3) != 0) return false;
        auto compiled = [&](const EwChain& c, const float* d) { EwChain probe = c; EwLoads ld; ew_plan_loads(probe, d, ld, EW_FWD_SLOTS_WIDE); return conv_gemm_chain_sig(probe) >= 0; };
        if (!compiled(ch, dst)) {
            // a network outside the signature table: without the resblock's Add the chain is [STORE raw,] MAXPAIR again (the Add keeps its kernel)
            if (k3 < 0) return false;
            ch.n = 0;
            if (keep_raw) push(ch, EW_STORE).pstore = e->T(o.d.out);
            push(ch, EW_MAXPAIR);
            dst = e->T(e->ops[o.pair_max].d.out);
            k3 = -1;
            if (!compiled(ch, dst)) return false;
        }
    }
    p.chain = ch;
    p.out0 = dst;
    p.chain_B = B;
    p.chain_eps = e->eps;
    e->fwd_done[o.pair_split] = 1;
    e->fwd_done[o.pair_max] = 1;
    if (k3 >= 0) { e->fwd_done[k3] = 1; e->pos_done[k3] = 1; }
    return true;
}

// lightcnn.py:252: `pool = MaxPool2d(2)(x) + AvgPool2d(2)(x)` -- MAXPOOL(k), AVGPOOL(k+1) on the same x, G_ADD(k+2) of the two, nobody else
// reading the pools' outputs: one pass over x writes the sum, the argmax bytes and (if the consumer's hook divides by it) the positive-pass sum,
// instead of max-pool, average pool (twice with the positive pass) and two adds.  Bit-identical (pool2_fwd_kernel).  false: nothing was launched.
static bool fuse_pool2_forward(xfr_engine* e, int k, int B, bool want_pos, hipStream_t s)
{
    if (!e->fuse_pools || k + 2 > e->fwd_last_op || k + 2 >= (int)e->ops.size()) return false;
    const xfr_op_desc& dm = e->ops[k].d;
    const xfr_op_desc& da = e->ops[k + 1].d;
    const xfr_op_desc& dd = e->ops[k + 2].d;
    if (da.kind != XFR_OP_AVGPOOL || dd.kind != XFR_OP_G_ADD || da.in0 != dm.in0) return false;
    if (!((dd.in0 == dm.out && dd.in1 == da.out) || (dd.in0 == da.out && dd.in1 == dm.out))) return false;
    if (dm.kh != 2 || dm.kw != 2 || dm.stride != 2 || dm.pad != 0 || da.kh != 2 || da.kw != 2 || da.stride != 2) return false;
    const Tensor& x = e->tens[dm.in0];
    const Tensor& tm = e->tens[dm.out];
    const Tensor& ta = e->tens[da.out];
    const Tensor& ts = e->tens[dd.out];
    if (tm.consumers.size() != 1 || ta.consumers.size() != 1 || ta.alias >= 0 || tm.need_pv) return false;
    uint8_t* idx = e->t_bank ? nullptr : e->idx_base() + e->ops[k].idx_off;
    if (!pool2_fwd_ok(e->T(dm.in0), idx, x.C * B, x.H, x.W, tm.H, tm.W)) return false;
    float* pos = nullptr;
    int relu_max = 0, avg_mode = 0;
    if (want_pos && ts.need_pv) {
        if (tm.pstate == PS_OTHER) return false;
        relu_max = tm.pstate == PS_RELU ? 1 : 0;
        avg_mode = ta.pstate == PS_EQ ? 0 : (ta.pstate == PS_RELU ? 1 : 2);
        if (avg_mode == 2 && x.nonneg) avg_mode = 0;          // the positive average pool clamps its input only where it is signed (pos_op)
        pos = e->Pv(dd.out);
    }
    launch_pool2_fwd(e->T(dm.in0), e->T(dd.out), idx, pos, x.C * B, x.H, x.W, tm.H, tm.W, relu_max, avg_mode, s);
    e->fwd_done[k + 1] = 1;
    e->fwd_done[k + 2] = 1;
    e->pos_done[k + 1] = 1;
    e->pos_done[k + 2] = 1;
    return true;
}

// forward of op k on true values (and, for "dual" convolutions, the positive output in the same launch)
static xfr_status fwd_op(xfr_engine* e, int k, int B, bool want_pos, hipStream_t s, bool keep_raw)
{
    OpRec& o = e->ops[k];
    const xfr_op_desc& d = o.d;
    const Tensor& a = e->tens[d.in0];
    const Tensor& t = e->tens[d.out];
    const long n_in = (long)B * a.per_n(), n_out = (long)B * t.per_n();
    switch (d.kind) {
        case XFR_OP_CONV:
        case XFR_OP_LINEAR: {
            ConvParams p;
            conv_geometry(e, k, B, p);
            p.in = e->T(d.in0);
            p.w = e->arena + o.w_true;
            p.bias = o.b_true >= 0 ? e->arena + o.b_true : nullptr;
            p.out0 = e->T(d.out);
            p.out1 = nullptr;
            p.CoutTot = d.cout;
            // dual launch: positive activations X = relu(W)*A + b from the same staged input tile.  Valid when the true
            // input is already A (provably >= 0).
            const bool dual = want_pos && t.need_pv && a.nonneg;
            if (dual) {
                p.w_pos = e->arena + o.w_pos;
                p.bias_pos = o.b_true >= 0 ? e->arena + (e->with_bias ? o.b_pos : o.b_true) : nullptr;
                p.out1 = e->Pv(d.out);
                p.nhalves = 2;
            } else p.nhalves = 1;
            // Light-CNN's first layer (one input channel, 5x5, MaxFeatureMap): a direct convolution instead of a 25-deep GEMM
            if (o.pair && e->fuse_fwd_only && e->direct_stem && !dual && !p.relu_in && a.C == 1 && d.kh == 5 && d.kw == 5 && d.stride == 1 && d.pad == 2 &&
                !o.tap_fwd && !o.tap4_fwd && o.pair_max <= e->fwd_last_op && !e->interpret_chains && stem5_mfm_ok(e->T(d.in0), B, a.H, a.W)) {
                if (!e->dry_run) launch_stem5_mfm(e->T(d.in0), p.w, o.ldw, p.bias, (want_pos || keep_raw) ? e->T(d.out) : nullptr, e->T(e->ops[o.pair_max].d.out), o.pair, B, a.H, a.W, s);
                e->fwd_done[o.pair_split] = 1;
                e->fwd_done[o.pair_max] = 1;
                return XFR_OK;
            }
            if (o.groups > 1) { }       // a grouped layer carries no epilogue: the ops behind it keep their kernels
            else if (o.pair && e->fuse_fwd_only && !dual && !p.relu_in && fuse_mfm_forward(e, k, B, want_pos || keep_raw, p, want_pos)) { }
            else if (!want_pos && e->fuse_fwd_only && !p.relu_in) fuse_forward_only(e, k, B, p, s);
            else if (want_pos && e->fuse_probe_fwd && !p.relu_in) fuse_probe_forward(e, k, B, p, s, dual);
            if (p.chain.n > 0 && p.chain.s[0].type == EW_LEAN_Q) {
                // one workgroup per tile accumulates W and relu(W) (the latter from the clamped W fragment): no second pack, no second output
                p.nhalves = 1;
                p.dualacc = 1;
                if (!e->dry_run) e->lean_launches++;
                p.w_pos = nullptr;
                p.out1 = nullptr;
            } else if (e->lean_cur && !e->lean_decide && e->lean_cur->lean_q[d.out] == 1) {
                return fail(XFR_STATE_ERROR, "lean schedule: convolution %d was planned with a lean epilogue and ran without one", k);
            }
            if (e->dry_run) return XFR_OK;
            return run_conv(e, p, s);
        }
        case XFR_OP_BATCHNORM:
            launch_affine_c(e->T(d.in0), e->T(d.out), e->arena + o.bn_alpha_t, e->arena + o.bn_beta_t, t.C, (long)B * t.HW(), 0,
                            o.fuse_relu ? 1 : 0, s);
            return XFR_OK;
        case XFR_OP_RELU:
            if (o.relu_fused_away) return XFR_OK;
            launch_relu(e->T(d.in0), e->T(d.out), n_in, s);
            return XFR_OK;
        case XFR_OP_MAXPOOL:
            if (fuse_pool2_forward(e, k, B, want_pos, s)) return XFR_OK;
            launch_maxpool_fwd(e->T(d.in0), e->T(d.out), e->t_bank ? nullptr : e->idx_base() + o.idx_off, a.C * B, a.H, a.W, t.H, t.W, d.kh, d.stride, d.pad, s);
            return XFR_OK;
        case XFR_OP_AVGPOOL: {
            if (t.alias >= 0) return XFR_OK;
            // the pooled shortcut lives inside its zero-padded form (layout_workspace): the pool writes the padding planes as well
            int zero_planes = 0;
            if (t.prefix_of >= 0 && e->hoist_shortcut && t.consumers[0] <= e->fwd_last_op) {
                zero_planes = (e->tens[t.prefix_of].C - t.C) * B;
                e->fwd_done[t.consumers[0]] = 1;
            }
            launch_avgpool_fwd(e->T(d.in0), e->T(d.out), a.C * B, a.H, a.W, t.H, t.W, d.kh, d.stride, 0, s, zero_planes);
            return XFR_OK;
        }
        case XFR_OP_ADD:
        case XFR_OP_G_ADD:
            launch_add2(e->T(d.in0), e->T(d.in1), e->T(d.out), n_out, 0, 0, o.fuse_relu ? 1 : 0, s);
            return XFR_OK;
        case XFR_OP_CONCAT:
            if (e->T(d.in0) != e->T(d.out)) launch_copy_acc(e->T(d.in0), e->T(d.out), n_in, 0, s);
            if (n_out > n_in) launch_fill(e->T(d.out) + n_in, n_out - n_in, 0.f, s);
            return XFR_OK;
        case XFR_OP_MULTIPLY:
            launch_scale(e->T(d.in0), e->T(d.out), n_in, d.fparam, 0, s);
            return XFR_OK;
        case XFR_OP_SPLIT:
            return XFR_OK;
        case XFR_OP_G_MAXHALVES:
            launch_maxhalves_fwd(e->T(d.in0), e->T(d.out), t.C, (long)B * t.HW(), 0, s);
            return XFR_OK;
        case XFR_OP_G_NORMALIZE:
            launch_normalize_fwd(e->T(d.in0), e->T(d.out), e->t_bank ? nullptr : e->misc() + o.norm_off, t.C, B, 0, s);
            return XFR_OK;
    }
    return fail(XFR_UNSUPPORTED_LAYER, "forward: unsupported kind %d", d.kind);
}

// positive pass for tensor out(k) (only called when need_pv and not produced by a dual launch)
static xfr_status pos_op(xfr_engine* e, int k, int B, hipStream_t s)
{
    OpRec& o = e->ops[k];
    const xfr_op_desc& d = o.d;
    const Tensor& a = e->tens[d.in0];
    const Tensor& t = e->tens[d.out];
    const long n_out = (long)B * t.per_n();
    switch (d.kind) {
        case XFR_OP_CONV:
        case XFR_OP_LINEAR: {
            ConvParams p;
            conv_geometry(e, k, B, p);
            p.in = e->T(d.in0);
            p.relu_in = a.nonneg ? 0 : 1;
            p.w = e->arena + o.w_pos;
            p.bias = o.b_true >= 0 ? e->arena + (e->with_bias ? o.b_pos : o.b_true) : nullptr;
            p.out0 = e->Pv(d.out);
            p.CoutTot = d.cout; p.nhalves = 1;
            return run_conv(e, p, s);
        }
        case XFR_OP_BATCHNORM:
            launch_affine_c(e->T(d.in0), e->Pv(d.out), e->arena + o.bn_alpha_p, e->arena + (e->with_bias ? o.bn_beta_pb : o.bn_beta_p),
                            t.C, (long)B * t.HW(), a.nonneg ? 0 : 1, 0, s);
            return XFR_OK;
        case XFR_OP_AVGPOOL:
            launch_avgpool_fwd(e->T(d.in0), e->Pv(d.out), a.C * B, a.H, a.W, t.H, t.W, d.kh, d.stride, a.nonneg ? 0 : 1, s);
            return XFR_OK;
        case XFR_OP_ADD: {
            const Tensor& b = e->tens[d.in1];
            launch_add2(e->T(d.in0), e->T(d.in1), e->Pv(d.out), n_out, a.nonneg ? 0 : 1, b.nonneg ? 0 : 1, 0, s);
            return XFR_OK;
        }
        case XFR_OP_G_ADD: {
            const Src x = pv_src(e, d.in0), y = pv_src(e, d.in1);
            launch_add2(x.p, y.p, e->Pv(d.out), n_out, x.relu, y.relu, 0, s);
            return XFR_OK;
        }
        case XFR_OP_G_MAXHALVES: {
            const Src x = pv_src(e, d.in0);
            launch_maxhalves_fwd(x.p, e->Pv(d.out), t.C, (long)B * t.HW(), x.relu, s);
            return XFR_OK;
        }
        case XFR_OP_G_NORMALIZE: {
            const Src x = pv_src(e, d.in0);
            launch_normalize_fwd(x.p, e->Pv(d.out), nullptr, t.C, B, x.relu, s);
            return XFR_OK;
        }
    }
    return fail(XFR_UNSUPPORTED_LAYER, "positive pass: kind %d cannot have a computed positive value", d.kind);
}

xfr_status forward_all(xfr_engine* e, const float* x_dev, int B, int last_tensor, bool with_pos, hipStream_t s, bool keep_raw)
{
    // xfr_engine_hold_forward: consecutive calls on the same input share one forward (slot 0, main bank only)
    const bool holdable = e->hold_forward && e->cur_slot == 0 && !e->t_bank;
    if (holdable && e->held_x == x_dev && e->held_B == B && e->held_last == last_tensor && e->held_stream == s &&
        (e->held_pos || !with_pos))
        return XFR_OK;
    if (holdable) with_pos = true;           // later calls of the group may need the positive pass
    e->held_x = nullptr;
    const Tensor& in = e->tens[0];
    if (e->dry_run) { }
    else if (e->u8_on) launch_u8hwc_to_cnhw(reinterpret_cast<const uint8_t*>(x_dev), e->T(0), B, in.C, in.HW(), e->u8_pre, s);
    else launch_nchw_to_cnhw(x_dev, e->T(0), B, in.C, in.HW(), s);
    const int last_op = e->tens[last_tensor].producer;
    e->fwd_done.assign(e->ops.size(), 0);
    e->pos_done.assign(e->ops.size(), 0);
    e->fwd_last_op = last_op;
    for (int k = 0; k <= last_op; ++k) {
        xfr_status st = XFR_OK;
        if (!e->fwd_done[k]) st = fwd_op(e, k, B, with_pos, s, keep_raw);
        if (st != XFR_OK) return st;
        if (with_pos) {
            const Tensor& t = e->tens[e->ops[k].d.out];
            const xfr_op_desc& d = e->ops[k].d;
            if (t.need_pv && !e->pos_done[k]) {
                const bool dual_done = (d.kind == XFR_OP_CONV || d.kind == XFR_OP_LINEAR) && e->tens[d.in0].nonneg;
                if (!dual_done) { st = pos_op(e, k, B, s); if (st != XFR_OK) return st; }
            }
        }
    }
    if (holdable) { e->held_x = x_dev; e->held_B = B; e->held_last = last_tensor; e->held_pos = with_pos; e->held_stream = s; }
    return XFR_OK;
}

void lean_prepare(xfr_engine* e, BwdPlan& plan, int B)
{
    if (plan.lean_state >= 0) return;
    plan.lean_state = 0;
    if (plan.plain || plan.fused_gemm.empty() || !e->fuse_probe_fwd || !e->fuse_gemm_epilogue || e->interpret_chains) return;
    const int nt = (int)e->tens.size();
    const int last_op = e->tens[plan.seed_tensor].producer;
    // dry run of the probe forward: the same decisions the real one takes, nothing launched
    e->lean_q_run.assign(nt, 0);
    e->lean_final_run.assign(nt, -1);
    e->lean_missing_sig = false;
    e->fwd_done.assign(e->ops.size(), 0);
    e->pos_done.assign(e->ops.size(), 0);
    e->fwd_last_op = last_op;
    {
        Scoped<bool> decide(e->lean_decide, true), dry(e->dry_run, true);
        for (int k = 0; k <= last_op; ++k) {
            const int kind = e->ops[k].d.kind;
            if (e->fwd_done[k] || (kind != XFR_OP_CONV && kind != XFR_OP_LINEAR)) continue;
            if (fwd_op(e, k, B, true, nullptr) != XFR_OK) e->lean_missing_sig = true;
        }
    }
    bool any = false;
    for (int t = 0; t < nt; ++t) any = any || e->lean_q_run[t] == 1;
    if (!any || e->lean_missing_sig) return;
    lean_rewrite_plan(e, plan);
}

// may this call take the lean schedule?  (B % 4: every lean epilogue is a float4 epilogue)
bool lean_applies(xfr_engine* e, BwdPlan& plan, int B, const SweepCtx& cx)
{
    if (!e->lean || (B & 3) != 0 || e->trace_on || cx.observing() || e->hold_forward || plan.plain) return false;
    if (!e->fuse_probe_fwd || !e->fuse_gemm_epilogue || e->interpret_chains) return false;
    lean_prepare(e, plan, B);
    return plan.lean_state == 1;
}

}  // namespace xfr
