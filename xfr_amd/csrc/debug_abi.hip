// debug_abi.hip -- the C ABI's xfr_debug_* entry points: single launches of the engine's kernels on the caller's tensors, for tests and measurements.
#include "engine_internal.h"

extern "C" {

xfr_status xfr_debug_u8_preprocess(xfr_engine* e, const uint8_t* x_u8_dev, int32_t n, float* out_nchw_dev, void* stream)
{
    if (!e || !x_u8_dev || !out_nchw_dev) return fail(XFR_INVALID_ARG, "null argument");
    xfr_status st = require_u8(e);
    if (st != XFR_OK) return st;
    if (n < 1 || n > e->max_batch) return fail(XFR_INVALID_ARG, "batch %d outside [1, %d]", n, e->max_batch);
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    const Tensor& in = e->tens[0];
    launch_u8hwc_to_cnhw(x_u8_dev, e->T(0), n, in.C, in.HW(), e->u8_pre, s);
    launch_cnhw_to_nchw(e->T(0), out_nchw_dev, n, in.C, in.HW(), s);
    HIP_TRY(hipGetLastError());
    e->held_x = nullptr;
    return fence_slot0(e, s);
}

// contrastive_tail's launches (without the blur) on the caller's tensor, with the sums and thresholds readable
xfr_status xfr_debug_contrast_tail(xfr_engine* e, const float* p_dev, int32_t c, int32_t n, int32_t hw, float percentile, double* sums_dev,
                                   float* thr_dev, float* contrast_dev, void* stream)
{
    if (!e || !p_dev || !contrast_dev)
        return fail(XFR_INVALID_ARG, "debug_contrast_tail: null argument (e %p, p_dev %p, contrast_dev %p)", (void*)e, (const void*)p_dev, (void*)contrast_dev);
    if (c < 1 || n < 1 || hw < 1 || n > 32767)
        return fail(XFR_INVALID_ARG, "debug_contrast_tail: c %d, n %d, hw %d: each at least 1, 2 n at most 65535", c, n, hw);
    if (!(percentile <= 100.f))
        return fail(XFR_INVALID_ARG, "debug_contrast_tail: percentile %g: at most 100, or below 0 for the plain contrastive form", (double)percentile);
    if (((uintptr_t)p_dev & 15) != 0)
        return fail(XFR_INVALID_ARG, "debug_contrast_tail: p_dev %p is not 16-byte aligned", (const void*)p_dev);
    {
        const uintptr_t p0 = (uintptr_t)p_dev, p1 = p0 + (size_t)c * 2 * n * hw * sizeof(float);
        const struct { const char* name; const void* ptr; size_t bytes; } outs[3] = {{"sums_dev", sums_dev, sizeof(double) * 2 * n},
                                                                                     {"thr_dev", thr_dev, sizeof(float) * n},
                                                                                     {"contrast_dev", contrast_dev, sizeof(float) * n * hw}};
        for (const auto& o : outs)
            if (o.ptr && (uintptr_t)o.ptr < p1 && p0 < (uintptr_t)o.ptr + o.bytes)
                return fail(XFR_INVALID_ARG, "debug_contrast_tail: %s %p (%zu bytes) overlaps p_dev %p", o.name, o.ptr, o.bytes, (const void*)p_dev);
    }
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    const bool truncated = percentile >= 0.f;
    const size_t ws_bytes = truncation_scratch_bytes(n), sums_bytes = sizeof(double) * 2 * n;      // both multiples of 8
    DevBuf<char> scratch;      // goes away with the call
    XFR_TRY(scratch.alloc(ws_bytes + sums_bytes + sizeof(float) * n));
    double* sums = sums_dev ? sums_dev : reinterpret_cast<double*>(scratch + ws_bytes);
    float* thr = !truncated ? nullptr : thr_dev ? thr_dev : reinterpret_cast<float*>(scratch + ws_bytes + sums_bytes);
    launch_sample_sums(p_dev, sums, c, 2 * n, hw, s);
    if (truncated) launch_truncation_threshold(p_dev, sums, percentile, thr, scratch.p, c, n, hw, s);
    launch_contrast(p_dev, sums, thr, contrast_dev, c, n, hw, s);
    hipError_t err = hipGetLastError();
    if (err == hipSuccess) err = hipStreamSynchronize(s);      // nothing reads the scratch when it goes
    if (err != hipSuccess) return fail(XFR_HIP_ERROR, "debug_contrast_tail: %s", hipGetErrorString(err));
    return XFR_OK;
}

xfr_status xfr_debug_conv(const float* in_dev, const float* w_host, const float* bias_host, float* out_dev, int32_t cin, int32_t h,
                          int32_t w, int32_t nb, int32_t cout, int32_t kh, int32_t kw, int32_t stride, int32_t pad, int32_t relu_in,
                          int32_t cfg, int32_t reps, float* ms_out)
{
    if (!in_dev || !w_host || !out_dev || cin < 1 || cout < 1 || kh < 1 || kw < 1 || stride < 1 || reps < 1)
        return fail(XFR_INVALID_ARG, "xfr_debug_conv: bad arguments");
    const int khw = kh * kw, K = cin * khw;
    const int ldw = (int)align_up(cout, 128);
    const bool tap = khw > 1 && (cin % 16 == 0) && khw <= 64;
    const bool tap4 = khw > 1 && (cin == 3 || cin == 4) && khw <= 60;
    const int Kf = tap4 ? 4 * khw : K;
    std::vector<float> host(align_up(Kf, 32) * (size_t)ldw, 0.f);
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int tp = 0; tp < khw; ++tp) {
                const size_t kk = forward_pack_row(tap4, tap, ci, tp, cin, khw);
                host[kk * ldw + co] = w_host[((size_t)co * cin + ci) * khw + tp];
            }
    DevBuf<float> wd, bd, affine;
    XFR_TRY(wd.alloc(host.size()));
    HIP_TRY(hipMemcpy(wd, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
    if (bias_host) {
        XFR_TRY(bd.alloc(cout));
        HIP_TRY(hipMemcpy(bd, bias_host, cout * sizeof(float), hipMemcpyHostToDevice));
    }
    ConvParams p;
    memset(&p, 0, sizeof(p));
    p.in = in_dev; p.w = wd; p.bias = bd; p.out0 = out_dev;
    p.Cin = cin; p.H = h; p.W = w; p.NB = nb; p.in_nb = nb; p.out_nb = nb;
    p.kh = kh; p.kw = kw; p.stride = stride; p.pad = pad;
    p.OH = (h + 2 * pad - kh) / stride + 1; p.OW = (w + 2 * pad - kw) / stride + 1;
    p.K = Kf; p.K_logical = K; p.M = nb * p.OH * p.OW; p.CoutTot = cout; p.nhalves = 1; p.ldw = ldw;
    p.relu_in = relu_in; p.out_H = p.OH; p.out_W = p.OW; p.out_stride = 1;
    p.in_bytes = (unsigned)((size_t)cin * nb * h * w * sizeof(float));
    p.tap_major = tap4 ? 2 : (tap ? 1 : 0); p.force_cfg = cfg % 100;
    // ONE tail workspace for every call of the process (null stream; never freed), its arrival counters zeroed when it is made and never again: like
    // a stream's workspace in the engine, it sees launches of different kernels and part counts one after the other, and a launch that left a counter
    // behind would break the next call's (tests/test_gpu_split_kparts.py)
    static float* tws = nullptr;
    if (!tws) {
        HIP_TRY(hipMalloc(&tws, XFR_TAIL_WS_BYTES + XFR_TAIL_MAX_TILES * sizeof(unsigned)));
        HIP_TRY(hipMemset(reinterpret_cast<char*>(tws) + XFR_TAIL_WS_BYTES, 0, XFR_TAIL_MAX_TILES * sizeof(unsigned)));
    }
    p.tail_ws = tws; p.tail_ws_bytes = XFR_TAIL_WS_BYTES;
    p.tail_cnt = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(tws) + XFR_TAIL_WS_BYTES);
    p.tail_force = (cfg / 10000) % 100;  // 0 heuristic, 1 off, S >= 2 forced
    // (cfg / 100) % 10 == 1: the lean probe-forward launch of a convolution behind BatchNorm + ReLU (forward.hip fuse_probe_forward) -- two accumulator
    // tiles (ConvParams::dualacc), the chain LEAN_Q, AFFINE_C (scale 1, shift 0), RELU, LEAN_STORE.  out_dev then holds TWO tensors: relu(conv(W) + b),
    // and behind it the stored quotient relu(conv(W) + b) / (relu(conv(relu W) + b) + 1e-16), sign bit set where the first is <= 0
    const bool lean = (cfg / 100) % 10 == 1;
    if (lean) {
        if (relu_in || (p.M & 3)) return fail(XFR_INVALID_ARG, "xfr_debug_conv: a lean launch reads a clamped input and needs M %% 4 == 0");
        std::vector<float> ab(2 * (size_t)cout, 0.f);
        std::fill(ab.begin(), ab.begin() + cout, 1.f);
        XFR_TRY(affine.alloc(ab.size()));
        HIP_TRY(hipMemcpy(affine, ab.data(), ab.size() * sizeof(float), hipMemcpyHostToDevice));
        p.dualacc = 1; p.bias_pos = bd; p.chain_B = nb; p.chain_eps = 1e-16f;
        EwChain& ch = p.chain;
        auto push = [&](int type) -> EwStep& { EwStep& q = ch.s[ch.n++]; memset(&q, 0, sizeof(q)); q.type = type; q.prior_sb = -1; return q; };
        push(EW_LEAN_Q);
        { EwStep& q = push(EW_AFFINE_C); q.p0 = affine; q.p1 = affine + cout; }
        push(EW_RELU);
        { EwStep& q = push(EW_LEAN_STORE); q.action = 0; q.pstore = out_dev + (size_t)cout * p.M; }
        if (conv_gemm_cannot_launch(p)) return fail(XFR_UNSUPPORTED_LAYER, "xfr_debug_conv: the lean chain has no compiled epilogue");
    }
    const bool split = (cfg % 100) == CFG_BF16X6;  // the bf16x6 kernel (layers it does not cover run the fp32 kernel the rules give, like in the engine)
    // the planes (K17) that a bf16x6 launch builds for this pack go before the pack does, on every way out
    struct ForgetSplit { const float* w; size_t bytes; ~ForgetSplit() { if (w) conv_gemm_forget_split(w, bytes); } } forget{split ? wd.p : nullptr, host.size() * sizeof(float)};
    Event a, b;
    XFR_TRY(a.create(true));
    XFR_TRY(b.create(true));
    const int nstreams = std::max(1, std::min(4, cfg / 1000000));     // > 1: the same launches on several streams at once
    p.tail_force = (cfg / 10000) % 100;
    // untimed warm-up: as many launches as are timed (at most 200).  The allocations and copies above left the device idle; one launch
    // does not bring the clocks back, and the first configuration of a sweep row then reads 5-12 % low (round 4: the same kernel measured
    // first and third in a row)
    for (int r = 0; r < std::max(1, std::min(reps, 200)); ++r) launch_conv_gemm(p, 0);
    float ms = 0.f;
    if (nstreams == 1) {
        HIP_TRY(hipEventRecord(a, 0));
        for (int r = 0; r < reps; ++r) launch_conv_gemm(p, 0);
        HIP_TRY(hipEventRecord(b, 0));
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipEventElapsedTime(&ms, a, b));
    } else {
        // every stream needs its own tail-balancing scratch; the outputs coincide (same values)
        Stream st[4];
        DevBuf<float> tw[4];
        ConvParams q[4];
        for (int i = 0; i < nstreams; ++i) {
            XFR_TRY(st[i].create());
            XFR_TRY(tw[i].alloc((XFR_TAIL_WS_BYTES + XFR_TAIL_MAX_TILES * sizeof(unsigned)) / sizeof(float)));
            q[i] = p;
            q[i].tail_ws = tw[i];
            q[i].tail_cnt = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(tw[i].p) + XFR_TAIL_WS_BYTES);
            HIP_TRY(hipMemset(q[i].tail_cnt, 0, XFR_TAIL_MAX_TILES * sizeof(unsigned)));
        }
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipEventRecord(a, 0));
        for (int i = 0; i < nstreams; ++i) HIP_TRY(hipStreamWaitEvent(st[i], a, 0));
        for (int r = 0; r < reps; ++r)
            for (int i = 0; i < nstreams; ++i) launch_conv_gemm(q[i], st[i]);
        for (int i = 0; i < nstreams; ++i) {
            Event e;
            XFR_TRY(e.create());
            HIP_TRY(hipEventRecord(e, st[i]));
            HIP_TRY(hipStreamWaitEvent(0, e, 0));
        }
        HIP_TRY(hipEventRecord(b, 0));
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipEventElapsedTime(&ms, a, b));
        ms /= nstreams;                       // per launch, all streams' launches counted
    }
    if (ms_out) *ms_out = ms / reps;
    HIP_TRY(hipGetLastError());
    return XFR_OK;
}

// one grouped launch (configuration 13 or 14) on the caller's pointers, as run_conv and the backward pass make them: no engine, no plan, no timing
xfr_status xfr_debug_conv_grouped(const float* in_dev, float* out0_dev, float* out1_dev, const float* w_host, const float* bias_host,
                                  const float* bias_pos_host, int32_t cin, int32_t cout, int32_t groups, int32_t h, int32_t w, int32_t nb, int32_t in_nb,
                                  int32_t out_nb, int32_t kh, int32_t kw, int32_t stride, int32_t pad, int32_t pad_dw, int32_t relu_in, int32_t nhalves,
                                  int32_t accumulate, int32_t out_stride, int32_t out_H, int32_t out_W, int32_t cfg, int32_t* cfg_out, int32_t* tile_out)
{
    if (cfg_out) *cfg_out = 0;
    if (tile_out) *tile_out = 0;
    if (!in_dev || !out0_dev || !w_host)
        return fail(XFR_INVALID_ARG, "debug_conv_grouped: null argument (in_dev %p, out0_dev %p, w_host %p)", (const void*)in_dev, (void*)out0_dev, (const void*)w_host);
    if (nhalves < 1 || nhalves > 2 || (nhalves == 2 && !out1_dev))
        return fail(XFR_INVALID_ARG, "debug_conv_grouped: nhalves %d, out1_dev %p: one half, or two with a second output", nhalves, (void*)out1_dev);
    if (cfg != 0 && cfg != CFG_GROUP && cfg != CFG_DEPTHWISE)
        return fail(XFR_INVALID_ARG, "debug_conv_grouped: cfg %d: 0 (as the engine picks), %d or %d", cfg, (int)CFG_GROUP, (int)CFG_DEPTHWISE);
    if (groups < 2 || cin < 1 || cout < 1 || cin % groups || cout % groups)
        return fail(XFR_INVALID_ARG, "debug_conv_grouped: cin %d, cout %d, groups %d: at least two groups that divide both", cin, cout, groups);
    if (h < 1 || w < 1 || kh < 1 || kw < 1 || stride < 1)
        return fail(XFR_INVALID_ARG, "debug_conv_grouped: h %d, w %d, kh %d, kw %d, stride %d: each at least 1", h, w, kh, kw, stride);
    if (nb < 1 || nb > in_nb || nb > out_nb)
        return fail(XFR_INVALID_ARG, "debug_conv_grouped: nb %d, in_nb %d, out_nb %d: a batch prefix of both tensors, at least 1", nb, in_nb, out_nb);
    if ((relu_in | accumulate) & ~1) return fail(XFR_INVALID_ARG, "debug_conv_grouped: relu_in %d, accumulate %d: flags, 0 or 1", relu_in, accumulate);
    const long nh = (long)h + 2L * pad - kh, nw = (long)w + 2L * ((long)pad + pad_dw) - kw;
    if (nh < 0 || nw < 0 || nh / stride + 1 > 32767 || nw / stride + 1 > 32767)
        return fail(XFR_INVALID_ARG, "debug_conv_grouped: pad %d, pad_dw %d leave no output (or more than 32767 rows or columns) of a %d x %d map under %d x %d taps",
                    pad, pad_dw, h, w, kh, kw);
    const int OH = (int)(nh / stride) + 1, OW = (int)(nw / stride) + 1;
    if ((out_H == 0) != (out_W == 0) || out_H < 0 || out_stride < 1 || (out_H == 0 && out_stride != 1) ||
        (out_H != 0 && ((long)(OH - 1) * out_stride >= out_H || (long)(OW - 1) * out_stride >= out_W)))
        return fail(XFR_INVALID_ARG, "debug_conv_grouped: out_stride %d, out_H %d, out_W %d do not hold the %d x %d outputs (0, 0: dense, stride 1)", out_stride, out_H,
                    out_W, OH, OW);
    if (out_H == 0) { out_H = OH; out_W = OW; }
    // the kernels index a tensor with 32-bit offsets
    if ((double)cin * in_nb * h * w >= 2147483648.0 || (double)cout * out_nb * out_H * out_W >= 2147483648.0 || (double)nb * OH * OW >= 2147483648.0)
        return fail(XFR_INVALID_ARG, "debug_conv_grouped: a tensor of 2^31 elements or more (cin %d, in_nb %d, %d x %d; cout %d, out_nb %d, %d x %d)", cin, in_nb, h, w,
                    cout, out_nb, out_H, out_W);
    const int G = groups, Ci = cin / G, Co = cout / G;
    if ((double)Ci * kh * kw >= 1048576.0) return fail(XFR_INVALID_ARG, "debug_conv_grouped: K = %d x %d x %d of one group is 2^20 or more", Ci, kh, kw);
    const int K = Ci * kh * kw;

    // the per-group packs, as the forward branch of pack_weights fills them (weights.hip)
    const size_t pack = group_pack_floats(G, Co, K);
    std::vector<float> host((size_t)nhalves * pack, 0.f);
    for (int co = 0; co < cout; ++co) {
        const int g = co / Co, col = co % Co;
        const float* src = w_host + (size_t)co * K;
        for (int kk = 0; kk < K; ++kk) {
            const size_t at = group_pack_index(g, col, kk, Co, K);
            host[at] = src[kk];
            if (nhalves == 2) host[pack + at] = src[kk] > 0.f ? src[kk] : 0.f;
        }
    }
    DevBuf<float> wd, bd, bpd;
    XFR_TRY(wd.alloc(host.size()));
    HIP_TRY(hipMemcpy(wd, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
    if (bias_host) {
        XFR_TRY(bd.alloc(cout));
        HIP_TRY(hipMemcpy(bd, bias_host, cout * sizeof(float), hipMemcpyHostToDevice));
    }
    if (bias_pos_host && nhalves == 2) {
        XFR_TRY(bpd.alloc(cout));
        HIP_TRY(hipMemcpy(bpd, bias_pos_host, cout * sizeof(float), hipMemcpyHostToDevice));
    }
    ConvParams p;
    memset(&p, 0, sizeof(p));
    p.in = in_dev; p.w = wd; p.w_pos = nhalves == 2 ? wd + pack : nullptr; p.bias = bd; p.bias_pos = bpd; p.out0 = out0_dev; p.out1 = nhalves == 2 ? out1_dev : nullptr;
    p.Cin = cin; p.H = h; p.W = w; p.NB = nb; p.in_nb = in_nb; p.out_nb = out_nb;
    p.kh = kh; p.kw = kw; p.stride = stride; p.pad = pad; p.pad_dw = pad_dw;
    p.OH = OH; p.OW = OW; p.K = K; p.K_logical = K; p.M = nb * OH * OW; p.CoutTot = cout; p.nhalves = nhalves; p.ldw = GROUP_ROWS;
    p.relu_in = relu_in; p.accumulate = accumulate; p.out_H = out_H; p.out_W = out_W; p.out_stride = out_stride;
    p.in_bytes = (unsigned)((size_t)cin * in_nb * h * w * sizeof(float));
    p.groups = G;
    int ran = 0;
    if (cfg != CFG_GROUP && launch_conv_depthwise(p, 0)) ran = CFG_DEPTHWISE;
    if (!ran && cfg == CFG_DEPTHWISE)
        return fail(XFR_UNSUPPORTED_LAYER, "debug_conv_grouped: a launch the depthwise kernel does not take (Ci %d, Co %d, %d x %d taps, %d x %d map): nothing was launched", Ci,
                    Co, kh, kw, h, w);
    if (!ran) {
        if (!launch_conv_group(p, 0)) return fail(XFR_UNSUPPORTED_LAYER, "debug_conv_grouped: a launch the grouped kernel does not take: nothing was launched");
        ran = CFG_GROUP;
    }
    hipError_t err = hipGetLastError();
    if (err == hipSuccess) err = hipStreamSynchronize(0);      // the packs go away with the call: nothing reads them then
    if (err != hipSuccess) return fail(XFR_HIP_ERROR, "debug_conv_grouped: %s", hipGetErrorString(err));
    if (cfg_out) *cfg_out = ran;
    if (tile_out) *tile_out = ran == CFG_DEPTHWISE ? conv_depthwise_last_tile() : 0;
    return XFR_OK;
}

xfr_status xfr_debug_conv_stamps(void* stamps_dev, int32_t capacity_workgroups)
{
    if (stamps_dev && (capacity_workgroups == 0 || (capacity_workgroups < 0 && -capacity_workgroups < 256)))
        return fail(XFR_INVALID_ARG, "xfr_debug_conv_stamps: capacity must be positive (or <= -256: sampled mode)");
    conv_gemm_set_stamps(reinterpret_cast<unsigned long long*>(stamps_dev), capacity_workgroups);
    return XFR_OK;
}

xfr_status xfr_debug_conv_log(void* log_dev, int32_t capacity, const char* dump_path)
{
    if (dump_path) {
        const int n = conv_gemm_dump_log(dump_path);
        if (n < 0) return fail(XFR_HIP_ERROR, "xfr_debug_conv_log: cannot write %s", dump_path);
    }
    conv_gemm_set_log(reinterpret_cast<unsigned long long*>(log_dev), capacity);
    return XFR_OK;
}

}  // extern "C"
