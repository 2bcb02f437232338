// inpaint_abi.hip -- the C ABI of inpainting-game scoring (include/xfr_amd.h: xfr_inpaint_*; python/xfr/inpainting_game/inpainting_game.py:12-197):
// argument checks, the level table, the batched sweep with its side stream.  The kernels are inpaint.hip.
#include "engine_internal.h"

struct InpaintState {
    hipStream_t s_gen = nullptr;                       // the hybrids of batch i + 1 are built here while batch i encodes
    hipEvent_t ev_in = nullptr, ev_ready[2] = {nullptr, nullptr}, ev_free[2] = {nullptr, nullptr};
    float* xbuf[2] = {nullptr, nullptr};               // two batches of network input, max_batch x in_c x H x W
    float* emb = nullptr;                              // max_batch x D embeddings of the running batch
    size_t emb_floats = 0;
    char* scratch = nullptr;                           // per map: the sort's keys, indices and running sums
    size_t scratch_cap = 0;
    uint8_t* first_on = nullptr;                       // n_maps x H x W
    size_t first_on_cap = 0;
};

namespace xfr {

void inpaint_release(xfr_engine* e)
{
    InpaintState* st = e->inpaint;
    if (!st) return;
    for (int k = 0; k < 2; ++k) {
        if (st->xbuf[k]) (void)hipFree(st->xbuf[k]);
        if (st->ev_ready[k]) (void)hipEventDestroy(st->ev_ready[k]);
        if (st->ev_free[k]) (void)hipEventDestroy(st->ev_free[k]);
    }
    if (st->ev_in) (void)hipEventDestroy(st->ev_in);
    if (st->s_gen) (void)hipStreamDestroy(st->s_gen);
    if (st->emb) (void)hipFree(st->emb);
    if (st->scratch) (void)hipFree(st->scratch);
    if (st->first_on) (void)hipFree(st->first_on);
    delete st;
    e->inpaint = nullptr;
}

}  // namespace xfr

namespace {

struct MaskArgs {
    const double* sal;
    int n_maps;
    const double* noise;
    double max_noise;
    int include_zero, method;
    const double* levels;
    int n_levels;
};

xfr_status inpaint_state(xfr_engine* e, InpaintState** out)
{
    if (!e->inpaint) e->inpaint = new InpaintState();
    InpaintState* st = e->inpaint;
    if (!st->s_gen) {
        HIP_TRY(hipStreamCreateWithFlags(&st->s_gen, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&st->ev_in, hipEventDisableTiming));
        for (int k = 0; k < 2; ++k) {
            HIP_TRY(hipEventCreateWithFlags(&st->ev_ready[k], hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&st->ev_free[k], hipEventDisableTiming));
        }
    }
    *out = st;
    return XFR_OK;
}

template <class T>
xfr_status grow(T** p, size_t* cap, size_t need)
{
    if (*cap >= need) return XFR_OK;
    if (*p) { HIP_TRY(hipDeviceSynchronize()); (void)hipFree(*p); *p = nullptr; *cap = 0; }
    HIP_TRY(hipMalloc(p, need * sizeof(T)));
    *cap = need;
    return XFR_OK;
}

// what every entry point checks before anything is launched; the thresholds of the levels (:53-56) as the kernels' table
xfr_status check_masks(xfr_engine* e, const MaskArgs& a, long h, long w, InpaintLevels* lv)
{
    if (!e) return fail(XFR_INVALID_ARG, "null engine");
    if (!a.sal || !a.levels) return fail(XFR_INVALID_ARG, "inpaint: null argument");
    if (a.n_maps < 1) return fail(XFR_INVALID_ARG, "inpaint: %d maps", a.n_maps);
    if (a.n_levels < 1 || a.n_levels > INPAINT_MAX_LEVELS)
        return fail(XFR_INVALID_ARG, "inpaint: %d levels, a first_on byte holds 1 to %d", a.n_levels, INPAINT_MAX_LEVELS);
    if (a.method != XFR_INPAINT_PERCENT_DENSITY && a.method != XFR_INPAINT_THRESHOLDS)
        return fail(XFR_INVALID_ARG, "inpaint: method %d is neither percent-density (0) nor explicit thresholds (1)", a.method);
    if (h < 1 || w < 1 || h * w > INPAINT_MAX_PIXELS) return fail(XFR_INVALID_ARG, "inpaint: maps of %ld x %ld pixels", h, w);
    if (!std::isfinite(a.max_noise)) return fail(XFR_INVALID_ARG, "inpaint: max_noise %g", a.max_noise);
    lv->n = a.n_levels;
    for (int l = 0; l < a.n_levels; ++l) {
        const double v = a.levels[l];
        if (a.method == XFR_INPAINT_PERCENT_DENSITY) {
            if (!(v >= 0.0 && v <= 100.0)) return fail(XFR_INVALID_ARG, "inpaint: percentile %g of level %d outside [0, 100]", v, l);
            if (l > 0 && v < a.levels[l - 1]) return fail(XFR_INVALID_ARG, "inpaint: unsorted percentiles, %g of level %d after %g", v, l, a.levels[l - 1]);
            lv->thr[l] = 1.0 - v / 100.0;                                                // :53
        } else {
            if (!std::isfinite(v)) return fail(XFR_INVALID_ARG, "inpaint: threshold %g of level %d", v, l);
            if (l > 0 && v > a.levels[l - 1]) return fail(XFR_INVALID_ARG, "inpaint: unsorted thresholds, %g of level %d after %g", v, l, a.levels[l - 1]);
            lv->thr[l] = v;
        }
    }
    if (a.method == XFR_INPAINT_PERCENT_DENSITY && a.levels[a.n_levels - 1] == 100.0) lv->thr[a.n_levels - 1] = 0.0;      // :55-56
    return XFR_OK;
}

// the masks of all maps into the state's first_on, on `s`, ordered behind whatever an earlier call left on the side stream
xfr_status run_masks(xfr_engine* e, InpaintState* st, const MaskArgs& a, const InpaintLevels& lv, long n, uint8_t* first_on, double* cdf, hipStream_t s)
{
    HIP_TRY(hipEventRecord(st->ev_in, st->s_gen));
    HIP_TRY(hipStreamWaitEvent(s, st->ev_in, 0));
    xfr_status rc = grow(&st->scratch, &st->scratch_cap, a.method == XFR_INPAINT_PERCENT_DENSITY ? (size_t)a.n_maps * inpaint_scratch_bytes(n) : (size_t)256);
    if (rc != XFR_OK) return rc;
    if (!first_on) {
        rc = grow(&st->first_on, &st->first_on_cap, (size_t)a.n_maps * n);
        if (rc != XFR_OK) return rc;
        first_on = st->first_on;
    }
    launch_inpaint_masks(a.sal, a.noise, a.max_noise, a.include_zero, a.method == XFR_INPAINT_PERCENT_DENSITY ? 1 : 0, lv, a.n_maps, n, st->scratch, first_on,
                         cdf, s);
    HIP_TRY(hipGetLastError());
    return XFR_OK;
}

xfr_status enter(xfr_engine* e, InpaintState** st)
{
    HIP_TRY(hipSetDevice(e->device));
    return inpaint_state(e, st);
}

}  // namespace

extern "C" {

xfr_status xfr_inpaint_score(xfr_engine* e, const double* sal_dev, int32_t n_maps, const double* noise_dev, double max_noise, int32_t include_zero,
                             int32_t method, const double* levels_host, int32_t n_levels, const float* orig_dev, const float* inpaint_dev,
                             const float* gal_orig_dev, const float* gal_inp_dev, int32_t encode_tensor, double* pg_dev, double* pr_dev,
                             uint8_t* cls_dev, void* stream)
{
    if (!e) return fail(XFR_INVALID_ARG, "null engine");
    const MaskArgs a{sal_dev, n_maps, noise_dev, max_noise, include_zero, method, levels_host, n_levels};
    InpaintLevels lv;
    xfr_status rc = check_masks(e, a, e->in_h, e->in_w, &lv);
    if (rc != XFR_OK) return rc;
    if (!orig_dev || !inpaint_dev || !gal_orig_dev || !gal_inp_dev || !pg_dev || !pr_dev || !cls_dev) return fail(XFR_INVALID_ARG, "inpaint: null argument");
    if (encode_tensor < 1 || encode_tensor >= (int)e->tens.size()) return fail(XFR_INVALID_ARG, "inpaint: bad tensor id %d", encode_tensor);
    if (!e->weights_loaded) return fail(XFR_STATE_ERROR, "weights not loaded");
    InpaintState* st = nullptr;
    rc = enter(e, &st);
    if (rc != XFR_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int B = e->max_batch, C = e->in_c;
    const long HW = (long)e->in_h * e->in_w;
    const size_t D = (size_t)e->tens[encode_tensor].per_n();
    for (int k = 0; k < 2; ++k)
        if (!st->xbuf[k]) HIP_TRY(hipMalloc(&st->xbuf[k], (size_t)B * C * HW * sizeof(float)));
    rc = grow(&st->emb, &st->emb_floats, (size_t)B * D);
    if (rc != XFR_OK) return rc;
    rc = run_masks(e, st, a, lv, HW, nullptr, nullptr, s);
    if (rc != XFR_OK) return rc;
    HIP_TRY(hipEventRecord(st->ev_in, s));                 // the masks, and the two images, which may still be in flight on the caller's stream
    HIP_TRY(hipStreamWaitEvent(st->s_gen, st->ev_in, 0));
    const long total = (long)n_maps * n_levels;
    const long n_batches = (total + B - 1) / B;
    bool used[2] = {false, false};
    auto generate = [&](long i) -> xfr_status {
        const int k = (int)(i & 1);
        if (used[k]) HIP_TRY(hipStreamWaitEvent(st->s_gen, st->ev_free[k], 0));      // the forward that last read this buffer
        launch_inpaint_blend(st->first_on, orig_dev, inpaint_dev, st->xbuf[k], C, HW, i * B, B, total, n_levels, st->s_gen);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(st->ev_ready[k], st->s_gen));
        return XFR_OK;
    };
    // whatever happens, the caller's stream ends up ordered behind the side stream: nothing of this call outlives what the caller enqueues next
    auto join = [&]() { if (hipEventRecord(st->ev_in, st->s_gen) == hipSuccess) (void)hipStreamWaitEvent(s, st->ev_in, 0); };
    rc = generate(0);
    for (long i = 0; rc == XFR_OK && i < n_batches; ++i) {
        const int k = (int)(i & 1);
        if (i + 1 < n_batches) {
            rc = generate(i + 1);
            if (rc != XFR_OK) break;
        }
        hipError_t he = hipStreamWaitEvent(s, st->ev_ready[k], 0);
        if (he != hipSuccess) { rc = fail(XFR_HIP_ERROR, "hipStreamWaitEvent failed: %s", hipGetErrorString(he)); break; }
        rc = xfr_forward(e, st->xbuf[k], B, encode_tensor, st->emb, s);
        if (rc != XFR_OK) break;
        he = hipEventRecord(st->ev_free[k], s);
        if (he != hipSuccess) { rc = fail(XFR_HIP_ERROR, "hipEventRecord failed: %s", hipGetErrorString(he)); break; }
        used[k] = true;
        const long lo = i * B, hi = std::min(total, (i + 1) * B);       // hybrids [lo, hi); anything beyond is padding
        launch_inpaint_dist(st->emb, (int)(hi - lo), gal_orig_dev, gal_inp_dev, (int)D, pg_dev + lo, pr_dev + lo, cls_dev + lo, s);
    }
    if (rc != XFR_OK) { const std::string why = g_err; join(); g_err = why; return rc; }
    HIP_TRY(hipGetLastError());
    return XFR_OK;
}

xfr_status xfr_inpaint_iou(xfr_engine* e, const double* sal_dev, int32_t n_maps, const double* noise_dev, double max_noise, int32_t include_zero,
                           int32_t method, const double* levels_host, int32_t n_levels, const uint8_t* gt_dev, int64_t* counts_dev, void* stream)
{
    if (!e) return fail(XFR_INVALID_ARG, "null engine");
    const MaskArgs a{sal_dev, n_maps, noise_dev, max_noise, include_zero, method, levels_host, n_levels};
    InpaintLevels lv;
    xfr_status rc = check_masks(e, a, e->in_h, e->in_w, &lv);
    if (rc != XFR_OK) return rc;
    if (!gt_dev || !counts_dev) return fail(XFR_INVALID_ARG, "inpaint: null argument");
    InpaintState* st = nullptr;
    rc = enter(e, &st);
    if (rc != XFR_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const long HW = (long)e->in_h * e->in_w;
    rc = run_masks(e, st, a, lv, HW, nullptr, nullptr, s);
    if (rc != XFR_OK) return rc;
    launch_inpaint_iou(st->first_on, gt_dev, HW, n_maps, n_levels, reinterpret_cast<long long*>(counts_dev), s);
    HIP_TRY(hipGetLastError());
    return XFR_OK;
}

xfr_status xfr_inpaint_debug_masks(xfr_engine* e, const double* sal_dev, int32_t n_maps, int32_t h, int32_t w, const double* noise_dev, double max_noise,
                                   int32_t include_zero, int32_t method, const double* levels_host, int32_t n_levels, uint8_t* first_on_dev,
                                   double* cdf_dev, void* stream)
{
    if (!e) return fail(XFR_INVALID_ARG, "null engine");
    const MaskArgs a{sal_dev, n_maps, noise_dev, max_noise, include_zero, method, levels_host, n_levels};
    InpaintLevels lv;
    xfr_status rc = check_masks(e, a, h, w, &lv);
    if (rc != XFR_OK) return rc;
    if (!first_on_dev) return fail(XFR_INVALID_ARG, "inpaint: null argument");
    InpaintState* st = nullptr;
    rc = enter(e, &st);
    if (rc != XFR_OK) return rc;
    return run_masks(e, st, a, lv, (long)h * w, first_on_dev, cdf_dev, (hipStream_t)stream);
}

xfr_status xfr_inpaint_debug_blends(xfr_engine* e, const double* sal_dev, int32_t n_maps, const double* noise_dev, double max_noise, int32_t include_zero,
                                    int32_t method, const double* levels_host, int32_t n_levels, const float* orig_dev, const float* inpaint_dev,
                                    int32_t first, int32_t count, float* out_dev, void* stream)
{
    if (!e) return fail(XFR_INVALID_ARG, "null engine");
    const MaskArgs a{sal_dev, n_maps, noise_dev, max_noise, include_zero, method, levels_host, n_levels};
    InpaintLevels lv;
    xfr_status rc = check_masks(e, a, e->in_h, e->in_w, &lv);
    if (rc != XFR_OK) return rc;
    if (!orig_dev || !inpaint_dev || !out_dev) return fail(XFR_INVALID_ARG, "inpaint: null argument");
    const long total = (long)n_maps * n_levels;
    if (first < 0 || count < 1 || (long)first + count > total || count > 65535)
        return fail(XFR_INVALID_ARG, "inpaint: hybrids [%d, %d + %d) of %ld, at most 65535 per call", first, first, count, total);
    InpaintState* st = nullptr;
    rc = enter(e, &st);
    if (rc != XFR_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const long HW = (long)e->in_h * e->in_w;
    rc = run_masks(e, st, a, lv, HW, nullptr, nullptr, s);
    if (rc != XFR_OK) return rc;
    launch_inpaint_blend(st->first_on, orig_dev, inpaint_dev, out_dev, e->in_c, HW, first, count, total, n_levels, s);
    HIP_TRY(hipGetLastError());
    return XFR_OK;
}

}  // extern "C"
