// inpaint_abi.hip -- the C ABI of inpainting-game scoring (include/xfr_amd.h: xfr_inpaint_*; python/xfr/inpainting_game/inpainting_game.py:12-197):
// argument checks, the level tables, the options of the _ex forms (per-map levels, the caller's totals, the Gaussian of soft-edged masks), the two
// ends of the batched sweep (probe_sweep.hip).  The kernels are inpaint.hip.  Every option travels to the device as a kernel argument, so the
// _ex forms block the host no more than the plain ones.
#include <vector>
#include "engine_internal.h"

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

static_assert(INPAINT_MAX_BLUR_RADIUS == XFR_INPAINT_MAX_BLUR_RADIUS, "the header states the kernels' limit");

// the options of a call as the kernels take them
struct Options {
    bool per_map = false;                              // one launch of the mask kernel per map: its own level table, its own total
    const double* totals = nullptr;
    std::vector<InpaintLevels> lv;                     // one table, or n_maps with levels_per_map
    InpaintBlur blur;                                  // r == 0: hard masks
};

// what every entry point checks before anything is launched; the thresholds of the levels (:53-56) as the kernels' table
xfr_status check_levels(const MaskArgs& a, const double* levels, InpaintLevels* lv);

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
    return check_levels(a, a.levels, lv);
}

// one row of n_levels levels
xfr_status check_levels(const MaskArgs& a, const double* levels, InpaintLevels* lv)
{
    lv->n = a.n_levels;
    for (int l = 0; l < a.n_levels; ++l) {
        const double v = levels[l];
        if (a.method == XFR_INPAINT_PERCENT_DENSITY) {
            if (!(v >= 0.0 && v <= 100.0)) return fail(XFR_INVALID_ARG, "inpaint: percentile %g of level %d outside [0, 100]", v, l);
            if (l > 0 && v < levels[l - 1]) return fail(XFR_INVALID_ARG, "inpaint: unsorted percentiles, %g of level %d after %g", v, l, levels[l - 1]);
            lv->thr[l] = 1.0 - v / 100.0;                                                // :53
        } else {
            if (!std::isfinite(v)) return fail(XFR_INVALID_ARG, "inpaint: threshold %g of level %d", v, l);
            if (l > 0 && v > levels[l - 1]) return fail(XFR_INVALID_ARG, "inpaint: unsorted thresholds, %g of level %d after %g", v, l, levels[l - 1]);
            lv->thr[l] = v;
        }
    }
    if (a.method == XFR_INPAINT_PERCENT_DENSITY && levels[a.n_levels - 1] == 100.0) lv->thr[a.n_levels - 1] = 0.0;      // :55-56
    return XFR_OK;
}

// check_masks, then the options (opt may be null: none).  blur_allowed: the entry point builds hybrids or soft masks
xfr_status check_call(xfr_engine* e, const MaskArgs& a, long h, long w, const xfr_inpaint_options* opt, bool blur_allowed, Options* o)
{
    o->lv.resize(1);
    o->blur.r = 0;
    xfr_status rc = check_masks(e, a, h, w, &o->lv[0]);
    if (rc != XFR_OK || !opt) return rc;
    if (opt->struct_size != (int32_t)sizeof(xfr_inpaint_options))
        return fail(XFR_INVALID_ARG, "inpaint: options of struct_size %d, this library's xfr_inpaint_options has %d bytes", opt->struct_size,
                    (int)sizeof(xfr_inpaint_options));
    if (opt->levels_per_map) {
        o->lv.resize(a.n_maps);
        for (int m = 1; m < a.n_maps; ++m) {
            rc = check_levels(a, a.levels + (size_t)m * a.n_levels, &o->lv[m]);
            if (rc != XFR_OK) return rc;
        }
    }
    if (opt->totals_host)
        for (int m = 0; m < a.n_maps; ++m)
            if (!(opt->totals_host[m] > 0.0) || !std::isfinite(opt->totals_host[m]))
                return fail(XFR_INVALID_ARG, "inpaint: total %g of map %d, a caller's sum must be positive and finite", opt->totals_host[m], m);
    o->totals = opt->totals_host;
    o->per_map = opt->levels_per_map || opt->totals_host;
    const int r = opt->blur_radius;
    if (r == 0) return XFR_OK;                                                           // blur_level_host is then ignored
    if (!blur_allowed) return fail(XFR_INVALID_ARG, "inpaint: blur_radius %d, this call is defined on hard masks (blur_radius 0)", r);
    if (r < 0 || r > INPAINT_MAX_BLUR_RADIUS)
        return fail(XFR_INVALID_ARG, "inpaint: blur_radius %d outside [0, %d] (XFR_INPAINT_MAX_BLUR_RADIUS)", r, INPAINT_MAX_BLUR_RADIUS);
    const double* k = opt->blur_kernel_host;
    if (!k) return fail(XFR_INVALID_ARG, "inpaint: blur_radius %d without blur_kernel_host", r);
    for (int j = 0; j <= 2 * r; ++j)
        if (!std::isfinite(k[j]) || k[j] < 0.0) return fail(XFR_INVALID_ARG, "inpaint: blur weight %g at tap %d, weights are finite and non-negative", k[j], j);
    for (int j = 1; j <= r; ++j)
        if (k[r - j] != k[r + j]) return fail(XFR_INVALID_ARG, "inpaint: asymmetric blur kernel, %g at tap %d and %g at tap %d", k[r - j], r - j, k[r + j], r + j);
    o->blur.r = r;
    for (int j = 0; j <= r; ++j) o->blur.half[j] = k[r - j];
    for (int l = 0; l < a.n_levels; ++l) o->blur.soft[l] = opt->blur_level_host ? (opt->blur_level_host[l] ? 1 : 0) : 1;
    return XFR_OK;
}

// the hybrids [first, first + rows) of the list into `out`
void blend(const Options& o, const uint8_t* first_on, const float* orig, const float* inpaint, float* out, xfr_engine* e, long first, int rows, long total,
           int n_levels, hipStream_t s)
{
    if (o.blur.r > 0) launch_inpaint_soft_blend(first_on, orig, inpaint, out, e->in_c, e->in_h, e->in_w, first, rows, total, n_levels, o.blur, s);
    else launch_inpaint_blend(first_on, orig, inpaint, out, e->in_c, (long)e->in_h * e->in_w, first, rows, total, n_levels, s);
}

// what a call that launched closes with
xfr_status finish() { HIP_TRY(hipGetLastError()); return XFR_OK; }

// What every entry point opens with.  check(): the refusals in their order -- the engine, the masks and the options, then the entry point's own
// pointers (args_ok); without h and w the maps have the engine's input size.  The entry point's further checks follow it, then masks(): the sweep's
// guard on the caller's stream and the masks of all maps there, into the state's first_on (or the caller's).
struct Call : SweepCall {
    MaskArgs a;
    Options o;
    long HW = 0;

    xfr_status check(xfr_engine* e, const MaskArgs& args, long h, long w, const xfr_inpaint_options* opt, bool blur_allowed, bool args_ok)
    {
        if (!e) return fail(XFR_INVALID_ARG, "null engine");
        a = args;
        HW = h * w;
        const xfr_status rc = check_call(e, a, h, w, opt, blur_allowed, &o);
        if (rc != XFR_OK) return rc;
        return args_ok ? XFR_OK : fail(XFR_INVALID_ARG, "inpaint: null argument");
    }
    xfr_status check(xfr_engine* e, const MaskArgs& args, const xfr_inpaint_options* opt, bool blur_allowed, bool args_ok)
    {
        return check(e, args, e ? e->in_h : 0, e ? e->in_w : 0, opt, blur_allowed, args_ok);
    }

    // [first, first + count) of the list of n_maps x n_levels entries, for the hooks that write one row per entry
    xfr_status check_range(int first, int count, const char* what) const
    {
        const long total = (long)a.n_maps * a.n_levels;
        if (first < 0 || count < 1 || (long)first + count > total || count > 65535)
            return fail(XFR_INVALID_ARG, "inpaint: %s [%d, %d + %d) of %ld, at most 65535 per call", what, first, first, count, total);
        return XFR_OK;
    }

    xfr_status masks(xfr_engine* e, void* stream, uint8_t* first_on = nullptr, double* cdf = nullptr)
    {
        xfr_status rc = enter(e, (hipStream_t)stream);
        if (rc != XFR_OK) return rc;
        const long n = HW;
        if (!e->inpaint) e->inpaint.reset(new InpaintState());
        InpaintState* st = e->inpaint.get();
        rc = st->scratch.grow(a.method == XFR_INPAINT_PERCENT_DENSITY ? (size_t)a.n_maps * inpaint_scratch_bytes(n) : (size_t)256);
        if (rc != XFR_OK) return rc;
        if (!first_on) {
            rc = st->first_on.grow((size_t)a.n_maps * n);
            if (rc != XFR_OK) return rc;
            first_on = st->first_on;
        }
        const int density = a.method == XFR_INPAINT_PERCENT_DENSITY ? 1 : 0;
        if (!o.per_map) {
            launch_inpaint_masks(a.sal, a.noise, a.max_noise, a.include_zero, density, o.lv[0], a.n_maps, n, st->scratch, first_on, cdf, s);
            return finish();
        }
        for (int m = 0; m < a.n_maps; ++m) {               // the map's table and total are arguments of its own launch
            launch_inpaint_masks(a.sal + (size_t)m * n, a.noise, a.max_noise, a.include_zero, density, o.lv[o.lv.size() > 1 ? m : 0], 1, n,
                                 st->scratch + (density ? (size_t)m * inpaint_scratch_bytes(n) : (size_t)0), first_on + (size_t)m * n,
                                 cdf ? cdf + (size_t)m * n : nullptr, s, o.totals ? o.totals[m] : 0.0);
            HIP_TRY(hipGetLastError());
        }
        return XFR_OK;
    }
};

}  // namespace

extern "C" {

xfr_status xfr_inpaint_score_ex(xfr_engine* e, const double* sal_dev, int32_t n_maps, const double* noise_dev, double max_noise, int32_t include_zero,
                                int32_t method, const double* levels_host, int32_t n_levels, const float* orig_dev, const float* inpaint_dev,
                                const float* gal_orig_dev, const float* gal_inp_dev, int32_t encode_tensor, double* pg_dev, double* pr_dev,
                                uint8_t* cls_dev, const xfr_inpaint_options* opt, void* stream)
{
    Call c;
    xfr_status rc = c.check(e, {sal_dev, n_maps, noise_dev, max_noise, include_zero, method, levels_host, n_levels}, opt, true,
                            orig_dev && inpaint_dev && gal_orig_dev && gal_inp_dev && pg_dev && pr_dev && cls_dev);
    if (rc != XFR_OK) return rc;
    if (encode_tensor < 1 || encode_tensor >= (int)e->tens.size()) return fail(XFR_INVALID_ARG, "inpaint: bad tensor id %d", encode_tensor);
    if (!e->weights_loaded) return fail(XFR_STATE_ERROR, "weights not loaded");
    rc = c.masks(e, stream);
    if (rc != XFR_OK) return rc;
    hipStream_t s = c.s;
    const int B = e->max_batch, D = (int)e->tens[encode_tensor].per_n();
    rc = sweep_side_follows(c.sw, s);                      // the masks, and the two images, which may still be in flight on the caller's stream
    if (rc != XFR_OK) return rc;
    const uint8_t* first_on = e->inpaint->first_on;
    const long total = (long)n_maps * n_levels;
    return run_sweep(e, c.sw, total, encode_tensor, s,
        [&](long i, float* x, hipStream_t side) { blend(c.o, first_on, orig_dev, inpaint_dev, x, e, i * B, B, total, n_levels, side); },
        [&](long i, const float* emb, hipStream_t) {
            const long lo = i * B, hi = std::min(total, (i + 1) * B);       // hybrids [lo, hi); anything beyond is padding
            launch_inpaint_dist(emb, (int)(hi - lo), gal_orig_dev, gal_inp_dev, D, pg_dev + lo, pr_dev + lo, cls_dev + lo, s);
        });
}

xfr_status xfr_inpaint_iou_ex(xfr_engine* e, const double* sal_dev, int32_t n_maps, const double* noise_dev, double max_noise, int32_t include_zero,
                              int32_t method, const double* levels_host, int32_t n_levels, const uint8_t* gt_dev, int64_t* counts_dev,
                              const xfr_inpaint_options* opt, void* stream)
{
    Call c;
    xfr_status rc = c.check(e, {sal_dev, n_maps, noise_dev, max_noise, include_zero, method, levels_host, n_levels}, opt, false, gt_dev && counts_dev);
    if (rc == XFR_OK) rc = c.masks(e, stream);
    if (rc != XFR_OK) return rc;
    launch_inpaint_iou(e->inpaint->first_on, gt_dev, c.HW, n_maps, n_levels, reinterpret_cast<long long*>(counts_dev), c.s);
    return finish();
}

xfr_status xfr_inpaint_debug_masks_ex(xfr_engine* e, const double* sal_dev, int32_t n_maps, int32_t h, int32_t w, const double* noise_dev,
                                      double max_noise, int32_t include_zero, int32_t method, const double* levels_host, int32_t n_levels,
                                      uint8_t* first_on_dev, double* cdf_dev, const xfr_inpaint_options* opt, void* stream)
{
    Call c;
    const xfr_status rc = c.check(e, {sal_dev, n_maps, noise_dev, max_noise, include_zero, method, levels_host, n_levels}, h, w, opt, false, first_on_dev);
    return rc != XFR_OK ? rc : c.masks(e, stream, first_on_dev, cdf_dev);
}

xfr_status xfr_inpaint_debug_blends_ex(xfr_engine* e, const double* sal_dev, int32_t n_maps, const double* noise_dev, double max_noise,
                                       int32_t include_zero, int32_t method, const double* levels_host, int32_t n_levels, const float* orig_dev,
                                       const float* inpaint_dev, int32_t first, int32_t count, float* out_dev, const xfr_inpaint_options* opt,
                                       void* stream)
{
    Call c;
    xfr_status rc = c.check(e, {sal_dev, n_maps, noise_dev, max_noise, include_zero, method, levels_host, n_levels}, opt, true,
                            orig_dev && inpaint_dev && out_dev);
    if (rc == XFR_OK) rc = c.check_range(first, count, "hybrids");
    if (rc == XFR_OK) rc = c.masks(e, stream);
    if (rc != XFR_OK) return rc;
    blend(c.o, e->inpaint->first_on, orig_dev, inpaint_dev, out_dev, e, first, count, (long)n_maps * n_levels, n_levels, c.s);
    return finish();
}

xfr_status xfr_inpaint_debug_soft_masks(xfr_engine* e, const double* sal_dev, int32_t n_maps, const double* noise_dev, double max_noise,
                                        int32_t include_zero, int32_t method, const double* levels_host, int32_t n_levels, int32_t h, int32_t w,
                                        const xfr_inpaint_options* opt, int32_t first, int32_t count, double* masks_dev, void* stream)
{
    Call c;
    xfr_status rc = c.check(e, {sal_dev, n_maps, noise_dev, max_noise, include_zero, method, levels_host, n_levels}, h, w, opt, true, masks_dev);
    if (rc == XFR_OK) rc = c.check_range(first, count, "masks");
    if (rc == XFR_OK) rc = c.masks(e, stream);
    if (rc != XFR_OK) return rc;
    if (c.o.blur.r == 0) {                                 // no options, or a radius of 0: every level hard, through the same kernel
        c.o.blur.half[0] = 1.0;
        for (int l = 0; l < n_levels; ++l) c.o.blur.soft[l] = 0;
    }
    launch_inpaint_soft_masks(e->inpaint->first_on, masks_dev, h, w, first, count, n_levels, c.o.blur, c.s);
    return finish();
}

xfr_status xfr_inpaint_score(xfr_engine* e, const double* sal_dev, int32_t n_maps, const double* noise_dev, double max_noise, int32_t include_zero,
                             int32_t method, const double* levels_host, int32_t n_levels, const float* orig_dev, const float* inpaint_dev,
                             const float* gal_orig_dev, const float* gal_inp_dev, int32_t encode_tensor, double* pg_dev, double* pr_dev,
                             uint8_t* cls_dev, void* stream)
{
    return xfr_inpaint_score_ex(e, sal_dev, n_maps, noise_dev, max_noise, include_zero, method, levels_host, n_levels, orig_dev, inpaint_dev, gal_orig_dev,
                                gal_inp_dev, encode_tensor, pg_dev, pr_dev, cls_dev, nullptr, stream);
}

xfr_status xfr_inpaint_iou(xfr_engine* e, const double* sal_dev, int32_t n_maps, const double* noise_dev, double max_noise, int32_t include_zero,
                           int32_t method, const double* levels_host, int32_t n_levels, const uint8_t* gt_dev, int64_t* counts_dev, void* stream)
{
    return xfr_inpaint_iou_ex(e, sal_dev, n_maps, noise_dev, max_noise, include_zero, method, levels_host, n_levels, gt_dev, counts_dev, nullptr, stream);
}

xfr_status xfr_inpaint_debug_masks(xfr_engine* e, const double* sal_dev, int32_t n_maps, int32_t h, int32_t w, const double* noise_dev, double max_noise,
                                   int32_t include_zero, int32_t method, const double* levels_host, int32_t n_levels, uint8_t* first_on_dev,
                                   double* cdf_dev, void* stream)
{
    return xfr_inpaint_debug_masks_ex(e, sal_dev, n_maps, h, w, noise_dev, max_noise, include_zero, method, levels_host, n_levels, first_on_dev, cdf_dev,
                                      nullptr, stream);
}

xfr_status xfr_inpaint_debug_blends(xfr_engine* e, const double* sal_dev, int32_t n_maps, const double* noise_dev, double max_noise, int32_t include_zero,
                                    int32_t method, const double* levels_host, int32_t n_levels, const float* orig_dev, const float* inpaint_dev,
                                    int32_t first, int32_t count, float* out_dev, void* stream)
{
    return xfr_inpaint_debug_blends_ex(e, sal_dev, n_maps, noise_dev, max_noise, include_zero, method, levels_host, n_levels, orig_dev, inpaint_dev, first,
                                       count, out_dev, nullptr, stream);
}

}  // extern "C"
