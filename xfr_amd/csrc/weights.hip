// weights.hip -- the packs of the weight arena: the forward pack and the flipped backward-data pack of every convolution / linear layer, each with its
// relu(W) twin, the biases and the BatchNorm folds, filled into a host vector (no device is touched); and the bf16 planes of the packs that the bf16x6
// kernel runs.  xfr_engine_load_weights (engine.hip) copies the vector into the arena.
#include "engine_internal.h"

namespace xfr {

xfr_status pack_weights(const xfr_engine* e, const xfr_tensor_view* w, std::vector<float>& host)
{
    host.assign(e->arena_floats, 0.f);
    for (size_t k = 0; k < e->ops.size(); ++k) {
        const OpRec& o = e->ops[k];
        const xfr_op_desc& d = o.d;
        if (d.kind == XFR_OP_CONV || d.kind == XFR_OP_LINEAR) {
            const xfr_tensor_view& wv = w[d.w_weight];
            const int khw = d.kh * d.kw;
            if (!wv.data || wv.numel != (int64_t)d.cout * (o.Cin / o.groups) * khw)
                return fail(XFR_INVALID_ARG, "op %zu: weight has %lld elements, expected %lld", k, (long long)wv.numel,
                            (long long)d.cout * (o.Cin / o.groups) * khw);
            if (o.groups > 1) {
                // A grouped layer, weight [cout][Ci][kh][kw] with Ci = Cin / groups: every pack of a dense layer per group, group after group, in the
                // layout of conv_group.hip (common.h: group_pack_index) -- K ordered ci-major, (ci, kh, kw) within the group, which is the weight's own
                // order; rows up to the next multiple of 4 and the columns of a ragged row block stay zero.  Output channel co = g Co + col belongs to
                // group g; in the backward-data packs the roles swap: row (col, flipped tap) of group g, column ci.
                const int G = o.groups, Ci = o.Cin / G, Co = d.cout / G;
                float* wt = host.data() + o.w_true;
                float* wp = host.data() + o.w_pos;
                for (int co = 0; co < d.cout; ++co) {
                    const int g = co / Co, col = co % Co;
                    const float* src = wv.data + (size_t)co * o.K;
                    for (int kk = 0; kk < o.K; ++kk) {
                        const size_t at = group_pack_index(g, col, kk, Co, o.K);
                        wt[at] = src[kk];
                        wp[at] = src[kk] > 0.f ? src[kk] : 0.f;
                    }
                    for (int ci = 0; ci < Ci; ++ci)
                        for (int a = 0; a < d.kh; ++a)
                            for (int b = 0; b < d.kw; ++b) {
                                const float v = src[(ci * d.kh + a) * d.kw + b];
                                if (o.w_bwd >= 0) {
                                    const size_t at = group_pack_index(g, ci, (col * d.kh + (d.kh - 1 - a)) * d.kw + (d.kw - 1 - b), Ci, o.Kb);
                                    host[o.w_bwd + at] = v > 0.f ? v : 0.f;
                                    host[o.w_bwd_true + at] = v;
                                }
                                for (const PhaseRec& ph : o.phases) {
                                    const int s = d.stride;
                                    if (a % s != ph.r || b % s != ph.c) continue;
                                    const int i2 = ph.ka - 1 - a / s, j2 = ph.kb - 1 - b / s;
                                    const size_t at = group_pack_index(g, ci, (col * ph.ka + i2) * ph.kb + j2, Ci, ph.K);
                                    host[ph.w_bwd + at] = v > 0.f ? v : 0.f;
                                    host[ph.w_bwd_true + at] = v;
                                }
                            }
                }
                if (d.w_bias >= 0) {
                    const xfr_tensor_view& bv = w[d.w_bias];
                    if (!bv.data || bv.numel != d.cout) return fail(XFR_INVALID_ARG, "op %zu: bad bias size", k);
                    for (int co = 0; co < d.cout; ++co) {
                        host[o.b_true + co] = bv.data[co];
                        host[o.b_pos + co] = bv.data[co] > 0.f ? bv.data[co] : 0.f;
                    }
                }
                continue;
            }
            float* wt = host.data() + o.w_true;
            float* wp = host.data() + o.w_pos;
            // forward pack: [k][co], k = (ci,kh,kw) or tap-major (kh,kw,ci)
            // column of output channel co in the forward pack: interleaved halves for MaxFeatureMap convolutions (OpRec::pair)
            auto col_of = [&](int co) { return o.pair ? (co % o.pair) * 2 + co / o.pair : co; };
            for (int co = 0; co < d.cout; ++co) {
                const float* src = wv.data + (size_t)co * o.K;
                const int col = col_of(co);
                for (int ci = 0; ci < o.Cin; ++ci)
                    for (int tp = 0; tp < khw; ++tp) {
                        const float v = src[ci * khw + tp];
                        const size_t kk = forward_pack_row(o.tap4_fwd, o.tap_fwd, ci, tp, o.Cin, khw);
                        wt[kk * o.ldw + col] = v;
                        wp[kk * o.ldw + col] = v > 0.f ? v : 0.f;   // relu(W): whitebox.py:319
                    }
            }
            if (o.w_bwd >= 0) {
                // backward-data pack of relu(W): [k' = (co, kh', kw')][ci] with the kernel flipped
                float* wb = host.data() + o.w_bwd;
                float* wbt = host.data() + o.w_bwd_true;
                for (int co = 0; co < d.cout; ++co)
                    for (int ci = 0; ci < o.Cin; ++ci)
                        for (int a = 0; a < d.kh; ++a)
                            for (int b = 0; b < d.kw; ++b) {
                                const float v = wv.data[(((size_t)co * o.Cin + ci) * d.kh + a) * d.kw + b];
                                const int a2 = d.kh - 1 - a, b2 = d.kw - 1 - b;
                                const size_t kk = (o.tap_bwd && d.stride == 1) ? (size_t)(a2 * d.kw + b2) * d.cout + co
                                                                               : (size_t)(co * d.kh + a2) * d.kw + b2;
                                wb[kk * o.ldb + ci] = v > 0.f ? v : 0.f;
                                wbt[kk * o.ldb + ci] = v;
                            }
            }
            // backward-data packs of a strided KxK layer, one per phase: the taps (r + s i, c + s j) of the kernel as a ka x kb kernel, flipped
            for (const PhaseRec& ph : o.phases) {
                float* wb = host.data() + ph.w_bwd;
                float* wbt = host.data() + ph.w_bwd_true;
                for (int co = 0; co < d.cout; ++co)
                    for (int ci = 0; ci < o.Cin; ++ci)
                        for (int i = 0; i < ph.ka; ++i)
                            for (int j = 0; j < ph.kb; ++j) {
                                const int a = ph.r + d.stride * i, b = ph.c + d.stride * j;
                                const float v = wv.data[(((size_t)co * o.Cin + ci) * d.kh + a) * d.kw + b];
                                const int i2 = ph.ka - 1 - i, j2 = ph.kb - 1 - j;
                                const size_t kk = ph.tap ? (size_t)(i2 * ph.kb + j2) * d.cout + co : (size_t)(co * ph.ka + i2) * ph.kb + j2;
                                wb[kk * o.ldb + ci] = v > 0.f ? v : 0.f;
                                wbt[kk * o.ldb + ci] = v;
                            }
            }
            if (d.w_bias >= 0) {
                const xfr_tensor_view& bv = w[d.w_bias];
                if (!bv.data || bv.numel != d.cout) return fail(XFR_INVALID_ARG, "op %zu: bad bias size", k);
                for (int co = 0; co < d.cout; ++co) {
                    host[o.b_true + col_of(co)] = bv.data[co];
                    host[o.b_pos + col_of(co)] = bv.data[co] > 0.f ? bv.data[co] : 0.f;   // whitebox.py:323 (with_bias)
                }
            }
        } else if (d.kind == XFR_OP_BATCHNORM) {
            const int C = e->tens[d.out].C;
            const xfr_tensor_view &g = w[d.w_weight], &b = w[d.w_bias], &m = w[d.w_mean], &v = w[d.w_var];
            if (!g.data || !b.data || !m.data || !v.data || g.numel != C || b.numel != C || m.numel != C || v.numel != C)
                return fail(XFR_INVALID_ARG, "op %zu: bad batchnorm parameter sizes", k);
            for (int c = 0; c < C; ++c) {
                // at::native inference batch norm: alpha = w * invstd, beta = b - mean * alpha
                const float invstd = 1.0f / sqrtf(v.data[c] + d.fparam);
                const float gp = g.data[c] > 0.f ? g.data[c] : 0.f;            // relu(gamma): whitebox.py:317-320
                const float bp = b.data[c] > 0.f ? b.data[c] : 0.f;
                const float at = g.data[c] * invstd, ap = gp * invstd;
                host[o.bn_alpha_t + c] = at;
                host[o.bn_beta_t + c] = b.data[c] - m.data[c] * at;
                host[o.bn_alpha_p + c] = ap;
                host[o.bn_beta_p + c] = b.data[c] - m.data[c] * ap;
                host[o.bn_beta_pb + c] = bp - m.data[c] * ap;
            }
        }
    }
    return XFR_OK;
}

// bf16 planes (K17) of every pack the bf16x6 kernel may be asked to run, built when the weights arrive instead of at a pack's first launch (round 5:
// the first step after a weight change stalled once per covered layer).  Layers, not launches: the geometry of one image decides.
void presplit_weights(xfr_engine* e)
{
    if (!e->arena || !e->weights_loaded || !e->split_mask) return;        // (packs that have their planes keep them)
    for (size_t k = 0; k < e->ops.size(); ++k) {
        const OpRec& o = e->ops[k];
        const xfr_op_desc& d = o.d;
        if ((d.kind != XFR_OP_CONV && d.kind != XFR_OP_LINEAR) || o.groups > 1) continue;        // (a grouped layer never runs the bf16x6 kernel)
        ConvParams p;
        conv_geometry(e, (int)k, 1, p);
        p.CoutTot = d.cout; p.nhalves = 1;
        if ((e->split_mask & 1) && conv_gemm_split_covers(p)) {
            (void)conv_gemm_presplit(p, e->arena + o.w_true, 0);
            (void)conv_gemm_presplit(p, e->arena + o.w_pos, 0);
        }
        if ((e->split_mask & 2) && k != 0 && d.stride == 1) {
            // the backward-data GEMM of a stride-1 convolution (bwd_conv_params): a convolution with the flipped, transposed pack
            const Tensor& a = e->tens[d.in0];
            const Tensor& t = e->tens[d.out];
            ConvParams q;
            memset(&q, 0, sizeof(q));
            q.Cin = t.C; q.H = t.H; q.W = t.W;
            q.kh = d.kh; q.kw = d.kw; q.stride = 1; q.pad = d.kh - 1 - d.pad; q.pad_dw = d.kw - d.kh;
            q.OH = a.H; q.OW = a.W; q.out_stride = 1;
            q.tap_major = o.tap_bwd ? 1 : 0;
            q.CoutTot = a.C; q.nhalves = 1; q.ldw = o.ldb; q.K = o.Kb;
            if (conv_gemm_split_covers(q)) {
                (void)conv_gemm_presplit(q, e->arena + o.w_bwd, 0);
                (void)conv_gemm_presplit(q, e->arena + o.w_bwd_true, 0);
            }
        }
    }
}

}  // namespace xfr
