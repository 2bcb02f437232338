// plan_fuse.hip -- cross-kernel fusion of the backward schedule (plan.hip: make_plan) and the lean rewrite of the fused one.  Device-free: the passes
// move symbolic steps (BwdStep::Sym) around; pointers only appear when a sweep resolves them (backward.hip: resolve_chain).
#include "engine_internal.h"

namespace xfr {
namespace {

typedef BwdStep::Sym Sym;

// ---------------------------------------------------------------------------------------------------------------
// Cross-kernel fusion of the backward schedule.
//   1. copy forwarding: a full-tensor gradient copy (Add / functional-add VJP) becomes an alias; the first later
//      writer that accumulated into the copy's destination instead adds the alias source in its chain (EW_ADDP).
//   2. chain -> chain: EW(a->b) followed by EW(b->c) becomes one launch (with an EW_STORE of b if b has other readers).
//   3. GEMM -> chain: a non-scattering backward-data GEMM whose output only feeds a chain runs that chain in its
//      epilogue, so the gradient between two GEMMs is never written to HBM un-hooked.
// ---- helpers shared by the fusion passes
Sym fuse_mk(int type, int t0)
{
    Sym s; s.type = type; s.action = 0; s.t0 = t0; s.x_t = -1; s.f = 0.f; s.op = -1; s.slot = -1; s.tap = false;
    return s;
}

// The chain heads and stores below reuse Sym's fields.  These constructors are the one place where the mapping is written down; resolve_chain
// (backward.hip) turns it into pointers, and make_plan's EW_MAXHALF_IN (plan.hip: t0 = the Split tensor, action = channels of one half) is the
// only overloaded head built elsewhere.
//
// EW_POOL2_IN, head of the pool pair's chain: the summed gradient of a pixel from its 2x2 window's gradient and argmax byte.
//   op = the max-pool op (whose argmax bytes the head reads), action = width of the full-resolution tensor
Sym fuse_pool2_head(int maxpool_op, int full_w)
{
    Sym h = fuse_mk(EW_POOL2_IN, -1);
    h.op = maxpool_op;
    h.action = full_w;
    return h;
}
// EW_AVGUP_IN, head of the chain behind a down-sampling block's compact strided GEMM(s): builds the block input's gradient per pixel.
//   op = width of the full-resolution tensor, slot = the tensor whose gradient region holds the compact GEMM result;
//   action = what the pooled shortcut tensor's hook does (HOOK_*), -1: a pooled shortcut without an observed hook, -2: no pooled source at all
//   (projection shortcut: the head only puts the compact sum on the even pixels); t0 / x_t = that hook's a / x tensors where it divides
Sym fuse_avgup_head(int full_w, int compact_t, int action, const Sym* pooled_hook = nullptr)
{
    Sym h = fuse_mk(EW_AVGUP_IN, -1);
    h.action = action;
    if (pooled_hook) {
        h.action = pooled_hook->action;
        if (h.action == HOOK_DIV) { h.t0 = pooled_hook->t0; h.x_t = pooled_hook->x_t; }     // otherwise p is not observed in this schedule
    }
    h.op = full_w;
    h.slot = compact_t;
    return h;
}
// EW_STORE: action 0 = store the running value into t0's gradient (fuse_mk(EW_STORE, t0)); the side branch of fuse_stage_head_branch adds
//   action 1 = save the running value (no destination: t0 = -1) and action 2 = store the branch's result into t0, then restore the saved value
Sym fuse_store_save()
{
    Sym s = fuse_mk(EW_STORE, -1);
    s.action = 1;
    return s;
}
Sym fuse_store_restore(int t0)
{
    Sym s = fuse_mk(EW_STORE, t0);
    s.action = 2;
    return s;
}

bool reads(const BwdStep& b, int t)
{
    if (b.kind != ST_ZERO && b.src_t == t) return true;
    for (const Sym& y : b.chain) if (y.type == EW_ADDP && y.t0 == t) return true;
    for (const Sym& y : b.chain) if (y.type == EW_AVGUP_IN && y.slot == t) return true;      // the compact GEMM result in t's gradient region
    if (b.accumulate && b.dst_t == t) return true;
    return false;
}
bool writes(const BwdStep& b, int t)
{
    if (b.dst_t == t) return true;
    for (const Sym& y : b.chain) if (y.type == EW_STORE && y.t0 == t) return true;
    return false;
}
// a backward-data GEMM that takes no chain: it scatters (a strided layer), or it is a grouped layer's (conv_group.hip has no epilogue)
bool scatter_conv(const xfr_engine* e, const BwdStep& b) { return b.kind == ST_CONV_BWD && (e->ops[b.op].d.stride != 1 || e->ops[b.op].groups > 1); }
// first step at or after `from` that reads or writes t (st.size(): none)
size_t next_touch(const std::vector<BwdStep>& st, size_t from, int t)
{
    size_t k = from;
    for (; k < st.size(); ++k)
        if (reads(st[k], t) || writes(st[k], t)) break;
    return k;
}
// does a step at or after `from` read t before one rewrites it?
bool read_again(const std::vector<BwdStep>& st, size_t from, int t)
{
    for (size_t k = from; k < st.size(); ++k) {
        if (reads(st[k], t)) return true;
        if (writes(st[k], t)) break;
    }
    return false;
}
// the chain's head expands a smaller gradient into the tensor the chain runs over: nothing can be put in front of it
bool expanding_head(const BwdStep& b)
{
    return !b.chain.empty() && (b.chain[0].type == EW_MAXHALF_IN || b.chain[0].type == EW_POOL2_IN || b.chain[0].type == EW_AVGUP_IN);
}
// does the chain store to or add from the gradient of t?
bool chain_touches(const std::vector<Sym>& chain, int t)
{
    for (const Sym& y : chain)
        if ((y.type == EW_STORE || y.type == EW_ADDP) && y.t0 == t) return true;
    return false;
}

// Pass 1: copy forwarding.
void fuse_copy_forwarding(xfr_engine* e, std::vector<BwdStep>& st)
{
    std::vector<BwdStep> out;
    std::vector<int> alias(e->tens.size(), -1);
    for (size_t i = 0; i < st.size(); ++i) {
        BwdStep b = st[i];
        // readers use the alias
        if (b.kind != ST_ZERO && b.src_t >= 0 && alias[b.src_t] >= 0) b.src_t = alias[b.src_t];
        const int d = b.dst_t;
        // ... or a channel-prefix slice (ConcatChannels VJP: rows [0, C_d) of the source, same row stride) whose first toucher is the in-place hook
        // flush of d: that launch then reads the source's rows directly
        const bool full_copy = b.kind == ST_COPY && d >= 0 && e->tens[d].C == e->tens[b.src_t].C && b.copy_elems_per_sb == e->tens[d].C;
        bool prefix_copy = false;
        if (b.kind == ST_COPY && !b.accumulate && d >= 0 && !full_copy && e->fuse_avgup && e->tens[b.src_t].C > e->tens[d].C &&
            b.copy_elems_per_sb == e->tens[d].C && e->tens[b.src_t].HW() == e->tens[d].HW()) {
            for (size_t j = i + 1; j < st.size(); ++j) {
                const BwdStep& c = st[j];
                if (c.dst_t == d || (c.kind != ST_ZERO && c.src_t == d) || writes(c, b.src_t)) {
                    prefix_copy = c.kind == ST_EW && c.src_t == d && c.dst_t == d && !c.accumulate && !writes(c, b.src_t);
                    break;
                }
            }
        }
        if (b.kind == ST_COPY && !b.accumulate && d >= 0 && (full_copy || prefix_copy)) {
            // forward only if every later accumulating writer of d can take an addend in its chain
            bool ok = true;
            for (size_t j = i + 1; j < st.size() && ok; ++j) {
                const BwdStep& c = st[j];
                if (c.dst_t == d) {
                    // a chain flushed IN PLACE on d (hooks of d where its producer is glue) reads the copy's source instead
                    if (!c.accumulate && c.kind == ST_EW && c.src_t == d) break;
                    if (!c.accumulate) { ok = false; break; }
                    if (!(c.kind == ST_EW || (c.kind == ST_CONV_BWD && !scatter_conv(e, c)))) ok = false;
                    break;   // after the first physical writer the tensor is real again
                }
            }
            if (ok) { alias[d] = b.src_t; continue; }
        }
        if (d >= 0 && alias[d] >= 0) {
            // first physical writer of an aliased tensor: it was an accumulate; turn it into "+ alias source"
            if (b.accumulate) {
                b.accumulate = 0;
                // (behind a MaxFeatureMap head: that step defines the gradient the chain starts from)
                b.chain.insert(b.chain.begin() + ((!b.chain.empty() && b.chain[0].type == EW_MAXHALF_IN) ? 1 : 0), fuse_mk(EW_ADDP, alias[d]));
                if (b.kind == ST_CONV_BWD) b.ew_t = d;
            }
            alias[d] = -1;
        }
        out.push_back(b);
    }
    st.swap(out);
}

// Pass 1b: Light-CNN's pool pair (lightcnn.py:252: maxpool(x) + avgpool(x), both 2x2 / 2 on the same x).  AVGPOOL_BWD(S -> D), accumulating
// MAXPOOL_BWD(S -> D) and the in-place hook chain of D (the two pools' tensor hooks on the accumulated gradient) become ONE chain launch
// whose head (EW_POOL2_IN) builds the summed gradient of a pixel from its window's gradient and argmax byte: D is written once
// instead of written, read-modified twice and read again (13 -> 9.3 tensor passes per pooling stage with the expanding chain behind it).
void fuse_pool_pair(xfr_engine* e, std::vector<BwdStep>& st)
{
    for (size_t i = 0; e->fuse_pools && i + 1 < st.size(); ++i) {
        const BwdStep av = st[i], mx = st[i + 1];
        if (av.kind != ST_AVGPOOL_BWD || mx.kind != ST_MAXPOOL_BWD || av.accumulate || !mx.accumulate) continue;
        if (av.src_t != mx.src_t || av.dst_t != mx.dst_t || av.dst_t < 0) continue;
        const xfr_op_desc& da = e->ops[av.op].d;
        const xfr_op_desc& dm = e->ops[mx.op].d;
        const Tensor& x = e->tens[av.dst_t];
        const Tensor& y = e->tens[dm.out];
        if (da.in0 != av.dst_t || dm.in0 != av.dst_t || da.kh != 2 || da.kw != 2 || da.stride != 2 || dm.kh != 2 || dm.kw != 2 || dm.stride != 2 || dm.pad != 0)
            continue;
        if ((x.W & 3) != 0 || (x.H & 1) != 0 || y.H * 2 != x.H || y.W * 2 != x.W || (e->ops[mx.op].idx_off & 3) != 0) continue;
        BwdStep f;
        f.kind = ST_EW;
        f.src_t = av.src_t;
        f.dst_t = av.dst_t;
        f.ew_t = av.dst_t;
        f.accumulate = 0;
        f.chain.push_back(fuse_pool2_head(mx.op, x.W));
        size_t drop = 1;
        if (i + 2 < st.size()) {
            const BwdStep& c = st[i + 2];
            // (no EW_AVGUP_IN head exists yet: the passes that build one run later)
            if (c.kind == ST_EW && c.src_t == av.dst_t && c.dst_t == av.dst_t && !c.accumulate && c.ew_t == av.dst_t && !expanding_head(c) &&
                c.chain.size() + 1 <= XFR_MAX_EW_STEPS) {
                f.chain.insert(f.chain.end(), c.chain.begin(), c.chain.end());
                drop = 2;
            }
        }
        st[i] = f;
        st.erase(st.begin() + i + 1, st.begin() + i + 1 + drop);
    }
}

// Pass 2b (GEMM-fused schedules only: no traces, priors or stores there).  Down-sampling residual block, shortcut = AvgPool2d(2) [+ ConcatChannels],
// main path entered through a 1x1 / stride 2 convolution (resnet.py:111-149).  Its block-input gradient D was built by five launches:
//   COPY S -> P (channel prefix), EW P (the pooled tensor's hook, in place), AVGPOOL_BWD P -> D, ..., CONV_BWD -> D (scatter, read-modify-write),
//   EW D -> E (the block input's hook chain).
// Now the GEMM leaves its result compact and the last launch builds D's value per pixel in its head (EW_AVGUP_IN): D is never written,
// three launches are gone and the GEMM stores rows instead of scattering dwords.
void fuse_downsample_avgpool(xfr_engine* e, std::vector<BwdStep>& st)
{
    for (size_t i0 = 0; i0 < st.size(); ++i0) {
        const BwdStep cp = st[i0];
        // (the slice copy may already have been forwarded into the pooled tensor's hook launch: EW S -> P, one hook)
        const bool fwd_hook = cp.kind == ST_EW && cp.src_t != cp.dst_t && cp.chain.size() == 1 && cp.chain[0].type == EW_HOOK && !cp.chain[0].tap &&
                              cp.ew_t == cp.dst_t;
        if ((cp.kind != ST_COPY && !fwd_hook) || cp.accumulate || cp.dst_t < 0 || cp.src_t < 0) continue;
        const int S = cp.src_t, P = cp.dst_t;
        const Tensor& tp = e->tens[P];
        if ((cp.kind == ST_COPY && cp.copy_elems_per_sb != tp.C) || e->tens[S].C < tp.C || e->tens[S].H != tp.H || e->tens[S].W != tp.W) continue;
        size_t i1 = next_touch(st, i0 + 1, P);
        if (i1 >= st.size()) continue;
        const Sym* pooled_hook = nullptr;
        size_t i2 = i1;
        if (fwd_hook) {
            pooled_hook = &cp.chain[0];
        } else if (st[i1].kind == ST_EW) {          // the pooled tensor's hook, in place
            const BwdStep& h = st[i1];
            if (h.src_t != P || h.dst_t != P || h.accumulate || h.chain.size() != 1 || h.chain[0].type != EW_HOOK || h.chain[0].tap) continue;
            pooled_hook = &h.chain[0];
            i2 = next_touch(st, i1 + 1, P);
            if (i2 >= st.size()) continue;
        }
        const BwdStep av = st[i2];
        if (av.kind != ST_AVGPOOL_BWD || av.src_t != P || av.accumulate || av.dst_t < 0) continue;
        const xfr_op_desc& da = e->ops[av.op].d;
        const int D = av.dst_t;
        const Tensor& td = e->tens[D];
        if (da.kh != 2 || da.kw != 2 || da.stride != 2 || da.pad != 0 || td.H != 2 * tp.H || td.W != 2 * tp.W || td.C != tp.C) continue;
        if (next_touch(st, i2 + 1, P) < st.size()) continue;          // nobody else wants the pooled gradient
        const size_t i3 = next_touch(st, i2 + 1, D);
        if (i3 >= st.size()) continue;
        const BwdStep& cv = st[i3];
        if (cv.kind != ST_CONV_BWD || cv.dst_t != D || !cv.accumulate || !cv.chain.empty()) continue;
        const xfr_op_desc& dc = e->ops[cv.op].d;
        if (dc.kh != 1 || dc.kw != 1 || dc.stride != 2 || dc.pad != 0 || dc.in0 != D || e->tens[dc.out].H != tp.H || e->tens[dc.out].W != tp.W) continue;
        if (e->ops[cv.op].groups > 1) continue;            // a grouped layer has no compact form
        const size_t i4 = next_touch(st, i3 + 1, D);
        if (i4 >= st.size()) continue;
        const BwdStep& ew = st[i4];
        if (ew.kind != ST_EW || ew.src_t != D || ew.dst_t == D || ew.accumulate || ew.ew_t != D || ew.chain.empty()) continue;
        if (expanding_head(ew)) continue;
        if ((int)ew.chain.size() + 1 > XFR_MAX_EW_STEPS) continue;
        bool bad = chain_touches(ew.chain, D) || chain_touches(ew.chain, S);
        if (next_touch(st, i4 + 1, D) < st.size()) {       // a later reader of D would want the tensor that is no longer written
            size_t k = next_touch(st, i4 + 1, D);
            if (reads(st[k], D)) bad = true;
        }
        for (size_t k = i0 + 1; k <= i4 && !bad; ++k)
            if (writes(st[k], S)) bad = true;            // S is now read where the chain runs
        if (bad) continue;
        BwdStep f = ew;
        f.src_t = S;
        f.chain.insert(f.chain.begin(), fuse_avgup_head(td.W, D, -1, pooled_hook));
        st[i4] = f;
        st[i3].compact = true;
        st[i3].accumulate = 0;
        // erase back to front
        st.erase(st.begin() + i2);
        if (i1 != i2) st.erase(st.begin() + i1);
        st.erase(st.begin() + i0);
        --i0;
    }
}

// Pass 2b'.  The same block input where the shortcut is a strided 1x1 projection (resnet50_128.py): ZERO D, CONV_BWD -> D (scatter), ...,
// CONV_BWD -> D (scatter), EW D -> E.  Both GEMMs now work on the compact grid (the second accumulates there: dense rows), the zero fill
// is gone and the chain's head puts the sum on the even pixels (EW_AVGUP_IN without a pooled source).
void fuse_downsample_projection(xfr_engine* e, std::vector<BwdStep>& st)
{
    for (size_t i0 = 0; i0 < st.size(); ++i0) {
        if (st[i0].kind != ST_ZERO || st[i0].dst_t < 0) continue;
        const int D = st[i0].dst_t;
        const Tensor& td = e->tens[D];
        std::vector<size_t> gemms;
        size_t k = next_touch(st, i0 + 1, D);
        bool ok = true;
        int gh = -1, gw = -1;
        while (k < st.size() && st[k].kind == ST_CONV_BWD) {
            const BwdStep& cv = st[k];
            const xfr_op_desc& dc = e->ops[cv.op].d;
            const Tensor& tg = e->tens[dc.out];
            if (cv.dst_t != D || !cv.accumulate || !cv.chain.empty() || e->ops[cv.op].groups > 1 || dc.kh != 1 || dc.kw != 1 || dc.stride != 2 || dc.pad != 0 || dc.in0 != D ||
                td.H != 2 * tg.H || td.W != 2 * tg.W || (gh >= 0 && (gh != tg.H || gw != tg.W))) { ok = false; break; }
            gh = tg.H; gw = tg.W;
            gemms.push_back(k);
            k = next_touch(st, k + 1, D);
        }
        if (!ok || gemms.empty() || k >= st.size()) continue;
        const BwdStep& ew = st[k];
        if (ew.kind != ST_EW || ew.src_t != D || ew.dst_t == D || ew.accumulate || ew.ew_t != D || ew.chain.empty()) continue;
        if (expanding_head(ew)) continue;
        if ((int)ew.chain.size() + 1 > XFR_MAX_EW_STEPS) continue;
        bool bad = chain_touches(ew.chain, D);
        {
            const size_t k2 = next_touch(st, k + 1, D);
            if (k2 < st.size() && reads(st[k2], D)) bad = true;
        }
        if (bad) continue;
        st[k].chain.insert(st[k].chain.begin(), fuse_avgup_head(td.W, D, -2));
        for (size_t q = 0; q < gemms.size(); ++q) {
            st[gemms[q]].compact = true;
            st[gemms[q]].accumulate = q == 0 ? 0 : 1;
        }
        st.erase(st.begin() + i0);
        --i0;
    }
}

// Pass 3b (after the GEMM -> chain merges of pass 1).  First block of a stage: the GEMM that produces the gradient of the block's Add output ends [.., STORE(t), relu] -> D, where D (the
// shortcut operand's gradient) and t (the main-path operand's) have different readers, and the main path's chain EW(t -> u) starts with the
// same relu.  Both then continue from relu(v): the chain runs on in the GEMM's epilogue as [.., relu, STORE(D), rest] -> u -- the signature of
// every other block's epilogue -- and the stand-alone launch is gone.
void fuse_stage_head_relu(xfr_engine* e, std::vector<BwdStep>& st)
{
    for (size_t i = 0; i < st.size(); ++i) {
        BwdStep& a = st[i];
        if (a.kind != ST_CONV_BWD || scatter_conv(e, a) || a.compact || a.accumulate || a.chain.size() < 2 || a.dst_t < 0) continue;
        const size_t n = a.chain.size();
        const Sym r1 = a.chain[n - 1], s1 = a.chain[n - 2];
        auto plain_relu = [](const Sym& y) { return y.type == EW_HOOK && y.action == HOOK_RELU && !y.tap; };
        if (!plain_relu(r1) || s1.type != EW_STORE) continue;
        const int t = s1.t0, D = a.dst_t;
        if (t == D || t < 0) continue;
        const size_t j = next_touch(st, i + 1, t);
        if (j >= st.size()) continue;
        const BwdStep c = st[j];
        if (c.kind != ST_EW || c.src_t != t || c.accumulate || c.dst_t == t || c.dst_t == D || c.chain.empty() || !plain_relu(c.chain[0])) continue;
        if (e->tens[c.ew_t].C != e->tens[D].C || e->tens[c.ew_t].HW() != e->tens[D].HW()) continue;
        bool bad = chain_touches(c.chain, D) || chain_touches(c.chain, t);
        const bool other_readers = read_again(st, j + 1, t);
        const int u = c.dst_t;
        for (size_t k = i + 1; k < j && !bad; ++k) {
            if (writes(st[k], u) || reads(st[k], u)) bad = true;
            for (const Sym& y : c.chain)
                if (y.type == EW_ADDP && writes(st[k], y.t0)) bad = true;
        }
        if (bad || n - 2 + (other_readers ? 1 : 0) + 1 + c.chain.size() > XFR_MAX_EW_STEPS) continue;
        std::vector<Sym> merged(a.chain.begin(), a.chain.begin() + (n - 2));
        if (other_readers) merged.push_back(s1);
        merged.push_back(c.chain[0]);
        merged.push_back(fuse_mk(EW_STORE, D));
        merged.insert(merged.end(), c.chain.begin() + 1, c.chain.end());
        a.chain = merged;
        a.ew_t = D;
        a.dst_t = u;
        st.erase(st.begin() + j);
    }
}

// Pass 3c.  First block of a stage with a PROJECTION shortcut (resnet50_128.py): the GEMM that produces the gradient of the block's Add output
// ends [.., mask, STORE(t), rest_s] -> D: D, the shortcut branch's gradient, continues in the epilogue, and t, the Add output's gradient, is
// stored for the main path, whose own hook chain EW(t -> u) = [rest_m] was a launch of its own.  Both chains start from the same value:
// [.., mask, SAVE, rest_m, STORE(u) + RESTORE, rest_s] -> D runs the main path's chain as a side branch on the saved value -- the same
// operations on the same operands, t is never written, the launch is gone.
void fuse_stage_head_branch(xfr_engine* e, std::vector<BwdStep>& st)
{
    for (size_t i = 0; i < st.size(); ++i) {
        BwdStep& a = st[i];
        if (a.kind != ST_CONV_BWD || scatter_conv(e, a) || a.compact || a.accumulate || a.dst_t < 0 || a.chain.empty()) continue;
        int k = -1;
        bool plain = true;
        for (size_t q = 0; q < a.chain.size(); ++q) {
            const Sym& y = a.chain[q];
            if (y.type == EW_STORE && y.action == 0 && k < 0) k = (int)q;
            else if (y.type == EW_STORE && y.action != 0) plain = false;                 // one branch per chain
            if (y.type == EW_MAXHALF_OUT || y.type == EW_MAXPAIR || y.type == EW_ADDP_CO || y.type == EW_FORK_POSADD) plain = false;
        }
        if (k < 0 || !plain) continue;
        const int t = a.chain[k].t0, D = a.dst_t;
        if (t < 0 || t == D) continue;
        const size_t j = next_touch(st, i + 1, t);
        if (j >= st.size()) continue;
        const BwdStep c = st[j];
        if (c.kind != ST_EW || c.src_t != t || c.accumulate || c.dst_t < 0 || c.dst_t == t || c.dst_t == D || c.chain.empty()) continue;
        if (e->tens[c.ew_t].C != e->tens[a.ew_t >= 0 ? a.ew_t : D].C || e->tens[c.ew_t].HW() != e->tens[a.ew_t >= 0 ? a.ew_t : D].HW()) continue;
        const int u = c.dst_t;
        bool bad = false;
        for (const Sym& y : c.chain) {
            if (y.type != EW_HOOK && y.type != EW_MASK && y.type != EW_SCALE_C && y.type != EW_SCALE && y.type != EW_RELU) bad = true;   // plain per-element steps only
            if (y.type == EW_HOOK && y.tap) bad = true;
        }
        if (!bad && read_again(st, j + 1, t)) bad = true;        // nobody else reads t before it is rewritten
        for (size_t q = i + 1; q < j && !bad; ++q)
            if (writes(st[q], u) || reads(st[q], u)) bad = true;
        if (chain_touches(a.chain, u)) bad = true;
        if (bad || a.chain.size() + 1 + c.chain.size() > (size_t)XFR_MAX_EW_STEPS) continue;
        std::vector<Sym> merged(a.chain.begin(), a.chain.begin() + k);
        merged.push_back(fuse_store_save());
        merged.insert(merged.end(), c.chain.begin(), c.chain.end());
        merged.push_back(fuse_store_restore(u));
        merged.insert(merged.end(), a.chain.begin() + k + 1, a.chain.end());
        a.chain = merged;
        st.erase(st.begin() + j);
    }
}

// Passes 2 + 3 to a fixed point: chain -> chain merges (pass 0), GEMM -> chain merges (pass >= 1), the MaxFeatureMap fan-out (pass 2).
void fuse_merge_to_fixed_point(xfr_engine* e, std::vector<BwdStep>& st, int pass)
{
    bool changed = true;
    while (changed) {
        changed = false;
        for (size_t i = 0; i < st.size() && !changed; ++i) {
            BwdStep& a = st[i];
            const bool a_ew = a.kind == ST_EW;
            const bool a_conv = pass >= 1 && a.kind == ST_CONV_BWD && !scatter_conv(e, a);
            if (!a_ew && !a_conv) continue;
            const int b_t = a.dst_t;
            if (b_t < 0) continue;
            bool tap_inside = false;
            for (const Sym& y : a.chain) if (y.tap) tap_inside = true;
            if (tap_inside) continue;                       // the tap launch is the last one
            const size_t j = next_touch(st, i + 1, b_t);
            if (j >= st.size()) continue;
            BwdStep& c = st[j];
            // an IN-PLACE chain on b_t (hooks flushed where the producer is glue) merges too: the merged launch simply ends in b_t
            bool inplace = c.kind == ST_EW && c.dst_t == b_t && !c.accumulate;
            // ... and so does a chain that stores its own intermediate value back into b_t on the way (a chain -> chain merge of an
            // in-place flush with its reader): that store is then the one b_t's later readers see
            bool restores = false;
            for (const Sym& y : c.chain) if (y.type == EW_STORE && y.t0 == b_t) { inplace = false; restores = true; }
            if (c.dst_t == b_t) restores = false;
            if (c.kind != ST_EW || c.src_t != b_t || (writes(c, b_t) && !inplace && !restores)) continue;
            // fan-out: GEMM (-> Co channels) followed by the chain whose head is the MaxFeatureMap VJP (over 2 * Co channels)
            bool fan = false;
            // ... or behind the chain launch whose head is the pool pair's VJP (1b): the Co-channel gradient between them never reaches HBM
            const bool a_pool = a_ew && !a.chain.empty() && a.chain[0].type == EW_POOL2_IN && !a.accumulate;
            if (pass == 2 && (a_conv || a_pool) && !c.chain.empty() && c.chain[0].type == EW_MAXHALF_IN && e->tens[c.ew_t].C == 2 * e->tens[b_t].C &&
                e->tens[c.ew_t].HW() == e->tens[b_t].HW() && (e->tens[b_t].HW() & 3) == 0) {
                fan = true;
                for (const Sym& y : a.chain) if (y.type == EW_MAXHALF_OUT) fan = false;
                for (size_t q = 1; q < c.chain.size(); ++q)
                    if (c.chain[q].type == EW_SCALE_C || c.chain[q].type == EW_AFFINE_C || c.chain[q].type == EW_FORK_POSBN) fan = false;   // per-channel
            }                                                                                                                        // parameters of row c
            if (!fan && (e->tens[c.ew_t].C != e->tens[b_t].C || e->tens[c.ew_t].HW() != e->tens[b_t].HW())) continue;
            // behind a fan-out the chain runs per half at channel c + h * Co, but the epilogue loads per-channel parameters at GEMM row
            // c: a chain with per-channel steps must not follow EW_MAXHALF_OUT (at the merge that creates the fan-out, above, or later)
            {
                bool a_fanned = false, c_perchan = false;
                for (const Sym& y : a.chain) if (y.type == EW_MAXHALF_OUT) a_fanned = true;
                for (const Sym& y : c.chain) if (y.type == EW_SCALE_C || y.type == EW_AFFINE_C || y.type == EW_FORK_POSBN) c_perchan = true;
                if (a_fanned && c_perchan) continue;
            }
            // does anything after j still read b_t?  (in place: later readers want the chain's result, which is what stays)
            const bool other_readers = !inplace && read_again(st, j + 1, b_t);
            // the merged launch runs at position i: nothing in (i, j) may write c's destination or read/write what the
            // merged chain stores
            const int u = c.dst_t;
            bool blocked = false;
            for (size_t k = i + 1; k < j; ++k)
                if (writes(st[k], u) || reads(st[k], u)) blocked = true;
            // ADDP sources of c must be final before position i
            for (const Sym& y : c.chain)
                if (y.type == EW_ADDP)
                    for (size_t k = i; k < j; ++k)
                        if (writes(st[k], y.t0)) blocked = true;
            if (blocked) continue;
            std::vector<Sym> merged = a.chain;
            if (a.accumulate) {
                // a accumulates into b_t (partial sums already there): fold as an addend, then continue
                merged.push_back(fuse_mk(EW_ADDP, b_t));
            }
            if ((other_readers || a.accumulate) && !inplace && !restores) merged.push_back(fuse_mk(EW_STORE, b_t));
            if (fan) {
                Sym f = c.chain[0];
                f.type = EW_MAXHALF_OUT;
                merged.push_back(f);
                merged.insert(merged.end(), c.chain.begin() + 1, c.chain.end());
            } else {
                merged.insert(merged.end(), c.chain.begin(), c.chain.end());
            }
            if (c.accumulate) merged.push_back(fuse_mk(EW_ADDP, u));
            if ((int)merged.size() > XFR_MAX_EW_STEPS) continue;
            a.chain = merged;
            a.dst_t = u;
            a.accumulate = 0;
            if (a.kind == ST_CONV_BWD) a.ew_t = b_t;
            st.erase(st.begin() + j);
            changed = true;
        }
    }
}

}  // namespace

// The fused schedules of a plan, built by the passes above in this order.  plan.fused: copy forwarding, the pool pair and chain -> chain merges only (what
// the observing sweeps run); plan.fused_gemm_nofan: + the down-sampling block rewrites and GEMM -> chain merges; plan.fused_gemm: + the MaxFeatureMap fan-out.
void fuse_plan(xfr_engine* e, BwdPlan& plan)
{
    std::vector<BwdStep> st = plan.steps;
    fuse_copy_forwarding(e, st);
    fuse_pool_pair(e, st);
    fuse_merge_to_fixed_point(e, st, 0);
    plan.fused = st;
    if (e->fuse_avgup) {
        fuse_downsample_avgpool(e, st);
        fuse_downsample_projection(e, st);
    }
    fuse_merge_to_fixed_point(e, st, 1);
    if (e->fuse_avgup) fuse_stage_head_relu(e, st);
    if (e->fuse_branch) fuse_stage_head_branch(e, st);
    plan.fused_gemm_nofan = st;
    fuse_merge_to_fixed_point(e, st, 2);
    plan.fused_gemm.swap(st);
}

// ---- the lean schedule ------------------------------------------------------------------------------------------------------------
// Every hook of a plain sweep (nothing observed: no trace, prior, capture or stored firing) needs less than its literal operands:
//   * a hook whose x IS its a (every Conv / Linear / pool / Concat / Add hook): a * relu(g) / (a + eps) is relu(g) where a > 0
//     and 0 where a = 0 -- one bit per element.  Where the tensor is the in-place ReLU output behind a lean BatchNorm, that bit is the sign bit of
//     the BatchNorm hook's stored quotient (HOOK_GATE_SIGN), otherwise the tensor itself is compared with 0 (HOOK_GATE);
//   * the BatchNorm hook (a = relu(W x + b), x = relu(relu(W) x + b)) and, in the modes that divide there, the in-place ReLU hook behind it: the
//     probe forward stored a / (x + eps) (forward.hip: fuse_probe_forward), the hook is relu(g) * q (HOOK_Q);
//   * ReLU masks and RELU-action hooks that the steps in front of them already imply are dropped.
// lean_prepare (forward.hip) decides per plan (dry run of the probe forward, then lean_rewrite_plan on plan.fused_gemm); the literal schedules stay what every
// observing call runs.
static void lean_rewrite_chain(xfr_engine* e, const BwdPlan& plan, std::vector<Sym>& chain)
{
    std::vector<Sym> out;
    // ReLU-output roots whose positivity some lean BatchNorm quotient read by THIS chain carries in its sign bit
    auto sign_source = [&](int root) -> int {
        for (const Sym& y : chain)
            if (y.type == EW_HOOK && y.action == HOOK_DIV && !y.tap && y.x_t == y.t0 && y.t0 >= 0 && plan.lean_q[y.t0] == 1 && plan.lean_final[y.t0] == root) return y.t0;
        return -1;
    };
    bool nonneg = false;           // g >= 0 is known here
    int gated = -1;                // root r: g == 0 wherever T(r) <= 0 is known here
    // a lean hook clamps g itself: a plain clamp right in front of it is dropped
    auto drop_clamp = [&]() {
        if (!out.empty() && (out.back().type == EW_RELU || (out.back().type == EW_HOOK && out.back().action == HOOK_RELU && !out.back().tap))) out.pop_back();
    };
    for (const Sym& y : chain) {
        Sym z = y;
        switch (y.type) {
            case EW_HOOK: {
                if (y.tap) { out.push_back(z); nonneg = false; gated = -1; break; }       // P[-2]: p is stored, literal
                if (y.action == HOOK_DIV && y.x_t >= 0 && plan.lean_q[y.x_t] == 1 && y.x_t == y.t0) {
                    z.action = HOOK_Q; z.x_t = -1;                                        // the quotient sits in T(t0)
                    drop_clamp(); out.push_back(z); nonneg = true;
                } else if (y.action == HOOK_DIV && y.x_t >= 0 && plan.lean_q[y.x_t] == 2 && e->root(y.x_t) == e->root(y.t0)) {
                    z.action = HOOK_Q; z.t0 = y.x_t; z.x_t = y.x_t;                       // the quotient sits in Pv(x_t); zero exactly where the ReLU output is
                    drop_clamp(); out.push_back(z); nonneg = true; gated = e->root(y.t0);
                } else if (y.action == HOOK_DIV && y.x_t < 0) {
                    const int r = e->root(y.t0);
                    if (gated == r) { if (!nonneg) { z.type = EW_RELU; z.t0 = -1; out.push_back(z); nonneg = true; } break; }
                    const int c = sign_source(r);
                    if (c >= 0) { z.action = HOOK_GATE_SIGN; z.t0 = c; } else z.action = HOOK_GATE;
                    drop_clamp(); out.push_back(z); nonneg = true; gated = r;
                } else if (y.action == HOOK_RELU) {
                    if (!nonneg) { out.push_back(z); nonneg = true; }
                } else if (y.action == HOOK_PASS) {
                    // nothing observed, nothing returned: no step
                } else {
                    out.push_back(z); nonneg = (y.action == HOOK_DIV); gated = -1;        // a literal dividing hook (x from another tensor): p / (x + eps) >= 0
                }
                break;
            }
            case EW_MASK: {
                const int r = e->root(y.t0);
                if (gated == r) break;
                const int c = sign_source(r);
                if (c >= 0) { z.action = 1; z.t0 = c; }
                out.push_back(z); gated = r;
                break;
            }
            case EW_RELU: if (!nonneg) { out.push_back(z); nonneg = true; } break;
            case EW_SCALE_C: out.push_back(z); break;                                     // relu(gamma) * invstd >= 0: signs and zeros stay
            case EW_SCALE: out.push_back(z); if (!(y.f > 0.f)) { nonneg = false; gated = -1; } break;
            case EW_STORE: out.push_back(z); if (y.action == 2) { nonneg = false; gated = -1; } break;      // the restored value is the branch point's
            default: out.push_back(z); nonneg = false; gated = -1; break;                 // ADDP, chain heads, fan-outs: anything may follow
        }
    }
    chain.swap(out);
}

// the lean schedule of a plan whose probe forward decided (forward.hip: lean_prepare) which tensors hold quotients
void lean_rewrite_plan(xfr_engine* e, BwdPlan& plan)
{
    plan.lean_q = e->lean_q_run;
    plan.lean_final = e->lean_final_run;
    plan.fused_gemm_lean = plan.fused_gemm;
    for (BwdStep& b : plan.fused_gemm_lean)
        if (!b.chain.empty()) lean_rewrite_chain(e, plan, b.chain);
    plan.lean_state = 1;
}

}  // namespace xfr
