// finish_abi.hip -- the C ABI of saliency finishing (include/xfr_amd.h: xfr_finish_saliency): argument checks, the workspace, the upload of the caller's
// totals and colour table, the launches on the caller's stream.  The kernels are finish.hip.  The call uses the engine for its device and error
// reporting only: no weights, and nothing of the probe sweep.
#include <cmath>
#include <cstring>
#include "engine_internal.h"

namespace {

static_assert(FINISH_MAX_DIM == XFR_FINISH_MAX_DIM && FINISH_MAX_MAPS == XFR_FINISH_MAX_MAPS, "the header states the kernels' limits");

// do [a, a + na) and [b, b + nb) (bytes) share a byte?
bool overlap(const void* a, size_t na, const void* b, size_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

// scipy.ndimage.zoom sizes its own output, round(in * zoom) with zoom = 1 / (in / out); _resize_cubic pads or crops when that is not `out`
bool zoom_keeps_size(int in, int out) { return std::llround((double)in * (1.0 / ((double)in / (double)out))) == (long long)out; }

}  // namespace

extern "C" {

xfr_status xfr_finish_saliency(xfr_engine* e, const float* maps_dev, int32_t n, int32_t h, int32_t w, int32_t out_h, int32_t out_w, const float* totals_host,
                               const uint8_t* probes_u8_dev, const double* jet_lut_host, double* sal_out_dev, uint8_t* overlay_out_dev, void* stream)
{
    if (!e) return fail(XFR_INVALID_ARG, "null engine");
    if (!maps_dev || !sal_out_dev) return fail(XFR_INVALID_ARG, "finish_saliency: null maps or null output");
    if (n < 1 || n > FINISH_MAX_MAPS) return fail(XFR_INVALID_ARG, "finish_saliency: %d maps, 1 to %d (XFR_FINISH_MAX_MAPS)", n, FINISH_MAX_MAPS);
    if (h < 1 || w < 1 || out_h < 1 || out_w < 1 || h > FINISH_MAX_DIM || w > FINISH_MAX_DIM || out_h > FINISH_MAX_DIM || out_w > FINISH_MAX_DIM)
        return fail(XFR_INVALID_ARG, "finish_saliency: maps of %d x %d to %d x %d, every axis 1 to %d (XFR_FINISH_MAX_DIM)", h, w, out_h, out_w, FINISH_MAX_DIM);
    if (out_h < h || out_w < w)
        return fail(XFR_INVALID_ARG, "finish_saliency: %d x %d to %d x %d has a shrinking axis (the Gaussian pre-filter of a shrinking resize stays on the host)",
                    h, w, out_h, out_w);
    const bool identity = out_h == h && out_w == w;
    if (!identity && (!zoom_keeps_size(h, out_h) || !zoom_keeps_size(w, out_w)))
        return fail(XFR_INVALID_ARG, "finish_saliency: %d x %d to %d x %d is a size the zoom rounds away from (the padded result stays on the host)", h, w, out_h, out_w);
    if (probes_u8_dev && !jet_lut_host) return fail(XFR_INVALID_ARG, "finish_saliency: probes without a colour table (jet_lut_host)");
    if (probes_u8_dev && !overlay_out_dev) return fail(XFR_INVALID_ARG, "finish_saliency: probes without an overlay output");
    if (!probes_u8_dev && overlay_out_dev) return fail(XFR_INVALID_ARG, "finish_saliency: an overlay output without probes");
    if (totals_host)
        for (int i = 0; i < n; ++i)
            if (!(totals_host[i] >= 0.0f) || std::isinf(totals_host[i]))
                return fail(XFR_INVALID_ARG, "finish_saliency: total %d is %g, not a finite sum of non-negative values", i, (double)totals_host[i]);
    const long n_in = (long)h * w, n_out = (long)out_h * out_w;
    const size_t maps_b = (size_t)n * n_in * sizeof(float), sal_b = (size_t)n * n_out * sizeof(double), img_b = (size_t)n * n_out * 3;
    if (overlap(maps_dev, maps_b, sal_out_dev, sal_b)) return fail(XFR_INVALID_ARG, "finish_saliency: the finished maps overlap the maps");
    if (probes_u8_dev && (overlap(probes_u8_dev, img_b, overlay_out_dev, img_b) || overlap(probes_u8_dev, img_b, sal_out_dev, sal_b) ||
                          overlap(overlay_out_dev, img_b, sal_out_dev, sal_b) || overlap(overlay_out_dev, img_b, maps_dev, maps_b)))
        return fail(XFR_INVALID_ARG, "finish_saliency: the overlays overlap the probes or a map buffer, or the probes the finished maps");

    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    if (!e->finish) e->finish.reset(new FinishState());
    FinishState* st = e->finish.get();
    if (!st->ev_done) XFR_TRY(st->ev_done.create());
    if (st->done_recorded) HIP_TRY(hipStreamWaitEvent(s, st->ev_done, 0));
    xfr_status rc = st->stats.grow((size_t)n * FINISH_STATS);
    if (rc == XFR_OK && !identity) rc = st->planes.grow((size_t)n * finish_plane_doubles(h, w));
    if (rc == XFR_OK && totals_host) rc = st->totals.grow((size_t)n);
    if (rc == XFR_OK && probes_u8_dev) rc = st->lut.grow(768);
    if (rc != XFR_OK) return rc;
    bool uploaded = false;
    if (totals_host) {
        HIP_TRY(hipMemcpyAsync(st->totals, totals_host, (size_t)n * sizeof(float), hipMemcpyHostToDevice, s));
        uploaded = true;
    }
    if (probes_u8_dev && !(st->lut_set && std::memcmp(st->lut_host, jet_lut_host, sizeof(st->lut_host)) == 0)) {
        st->lut_set = false;
        std::memcpy(st->lut_host, jet_lut_host, sizeof(st->lut_host));
        HIP_TRY(hipMemcpyAsync(st->lut, st->lut_host, sizeof(st->lut_host), hipMemcpyHostToDevice, s));
        uploaded = true;
    }
    if (uploaded) HIP_TRY(hipStreamSynchronize(s));    // the caller's arrays go away with the call
    if (probes_u8_dev) st->lut_set = true;

    launch_finish_head(maps_dev, n, n_in, totals_host ? st->totals : nullptr, st->stats, s);
    if (identity) {
        launch_finish_identity(maps_dev, n, n_in, st->stats, sal_out_dev, s);
    } else {
        launch_finish_prefilter(maps_dev, n, h, w, st->stats, st->planes, s);
        launch_finish_resize(st->planes, n, h, w, out_h, out_w, st->stats, sal_out_dev, s);
    }
    if (probes_u8_dev) launch_finish_overlay(sal_out_dev, probes_u8_dev, n, n_out, st->stats, st->lut, overlay_out_dev, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(st->ev_done, s));
    st->done_recorded = true;
    return XFR_OK;
}

}  // extern "C"
