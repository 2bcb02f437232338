// strise_abi.hip -- the C ABI of STRise blackbox saliency (include/xfr_amd.h: xfr_strise_*; python/xfr/models/blackbox.py:299-442): argument checks,
// the two ends of the batched sweep (probe_sweep.hip), the grouping of the masks by shift for the merge.  The kernels are strise.hip.
#include "engine_internal.h"

struct StriseState {
    double* orig = nullptr;                            // n_refs + n_gal similarities of the unmasked probe, then as many 1 / |g|
    size_t orig_cap = 0;
    int* tab = nullptr;                                // cells, shifts, shift order and group offsets of the current call
    size_t tab_cap = 0;
    double* merge_ws = nullptr;                        // A [scale^2][gh * gw] and wsum [scale^2]
    size_t merge_cap = 0;
};

namespace xfr {

void strise_release(xfr_engine* e)
{
    StriseState* st = e->strise;
    if (!st) return;
    if (st->orig) (void)hipFree(st->orig);
    if (st->tab) (void)hipFree(st->tab);
    if (st->merge_ws) (void)hipFree(st->merge_ws);
    delete st;
    e->strise = nullptr;
}

}  // namespace xfr

namespace {

StriseState* strise_state(xfr_engine* e)
{
    if (!e->strise) e->strise = new StriseState();
    return e->strise;
}

// what every entry point checks before anything is launched
xfr_status check_masks(xfr_engine* e, const int32_t* cells, const int32_t* shifts, int n_masks, const xfr_strise_geometry* geom, StriseGeom* g)
{
    if (!e) return fail(XFR_INVALID_ARG, "null engine");
    if (!cells || !shifts || !geom) return fail(XFR_INVALID_ARG, "strise: null argument");
    if (n_masks < 1) return fail(XFR_INVALID_ARG, "strise: %d masks", n_masks);
    if (geom->grid_h < 1 || geom->grid_w < 1 || geom->mask_scale < 1 || geom->num_elements < 1)
        return fail(XFR_INVALID_ARG, "strise: grid %d x %d, mask_scale %d, %d elements per mask", geom->grid_h, geom->grid_w, geom->mask_scale, geom->num_elements);
    // a shift lies inside one cell of the image: a larger scale is no mask geometry, and scale^2 shift groups size the merge's workspace and grid
    if (geom->mask_scale > e->in_h || geom->mask_scale > e->in_w)
        return fail(XFR_INVALID_ARG, "strise: mask_scale %d exceeds the %d x %d input", geom->mask_scale, e->in_h, e->in_w);
    const long nc = (long)geom->grid_h * geom->grid_w;
    if (nc > STRISE_MAX_CELLS) return fail(XFR_INVALID_ARG, "strise: a grid of %d x %d cells exceeds %d", geom->grid_h, geom->grid_w, STRISE_MAX_CELLS);
    if (geom->num_elements > nc) return fail(XFR_INVALID_ARG, "strise: %d elements per mask in a grid of %ld cells", geom->num_elements, nc);
    for (long i = 0; i < (long)n_masks * geom->num_elements; ++i)
        if (cells[i] < 0 || cells[i] >= nc)
            return fail(XFR_INVALID_ARG, "strise: cell index %d of mask %ld outside the %d x %d grid", cells[i], i / geom->num_elements, geom->grid_h, geom->grid_w);
    for (long i = 0; i < 2L * n_masks; ++i)
        if (shifts[i] < 0 || shifts[i] >= geom->mask_scale)
            return fail(XFR_INVALID_ARG, "strise: shift %d of mask %ld outside [0, %d)", shifts[i], i / 2, geom->mask_scale);
    *g = StriseGeom{e->in_h, e->in_w, geom->grid_h, geom->grid_w, geom->mask_scale, geom->num_elements,
                    (double)geom->grid_h / (double)(e->in_h + geom->mask_scale), (double)geom->grid_w / (double)(e->in_w + geom->mask_scale)};
    return XFR_OK;
}

// only the arithmetic of convert_resnet101v4_image is built into the masked-probe kernel
xfr_status check_u8(xfr_engine* e)
{
    if (e->in_c != 3 || !e->u8_set || e->u8_pre.kind != XFR_U8_SUB_MEAN || e->u8_pre.channels != 3)
        return fail(XFR_INVALID_ARG, "strise: masked probes need a 3-channel network with XFR_U8_SUB_MEAN preprocessing of 3-channel images "
                                     "(xfr_engine_set_u8_preprocess); this engine takes %d channels", e->in_c);
    return XFR_OK;
}

// a host table into the state's `tab` on `s`; the host waits for the copy there: the table is pageable and local to the call
xfr_status upload_table(StriseState* st, const std::vector<int>& tab, hipStream_t s)
{
    xfr_status rc = grow(&st->tab, &st->tab_cap, tab.size());
    if (rc != XFR_OK) return rc;
    HIP_TRY(hipMemcpyAsync(st->tab, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    return XFR_OK;
}

// rows [first, first + count) of the sweep's image list -- image 0 is the unmasked probe, images 1 .. n_masks the masks, anything beyond is padding
// (all-ones masks: cell -1, shift 0) -- as one table on the device: count x n_elem cells, then count x 2 shifts
xfr_status upload_rows(StriseState* st, const int32_t* cells, const int32_t* shifts, int n_masks, int n_elem, long first, long count, bool with_probe,
                       hipStream_t s)
{
    std::vector<int> tab((size_t)count * (n_elem + 2), -1);
    int* sh = tab.data() + (size_t)count * n_elem;
    for (long r = 0; r < count; ++r) {
        const long k = first + r - (with_probe ? 1 : 0);
        if (k >= 0 && k < n_masks) {
            memcpy(tab.data() + (size_t)r * n_elem, cells + (size_t)k * n_elem, sizeof(int) * n_elem);
            sh[2 * r] = shifts[2 * k];
            sh[2 * r + 1] = shifts[2 * k + 1];
        } else {
            sh[2 * r] = sh[2 * r + 1] = 0;
        }
    }
    return upload_table(st, tab, s);
}

}  // namespace

extern "C" {

xfr_status xfr_strise_score(xfr_engine* e, const uint8_t* probe_u8_dev, const double* fill_dev, const int32_t* cells_host, const int32_t* shifts_host,
                            int32_t n_masks, const xfr_strise_geometry* geom, const float* refs_dev, int32_t n_refs, const float* gallery_dev,
                            int32_t n_gal, int32_t encode_tensor, double* scores_dev, double* orig_dev, void* stream)
{
    StriseGeom g;
    xfr_status rc = check_masks(e, cells_host, shifts_host, n_masks, geom, &g);
    if (rc != XFR_OK) return rc;
    if (!probe_u8_dev || !fill_dev || !refs_dev || !gallery_dev || !scores_dev) return fail(XFR_INVALID_ARG, "strise: null argument");
    rc = check_u8(e);
    if (rc != XFR_OK) return rc;
    if (n_refs < 1 || n_gal < 1 || (n_refs != n_gal && n_refs != 1 && n_gal != 1))
        return fail(XFR_INVALID_ARG, "strise: %d references against %d gallery images do not broadcast (equal counts, or one of them 1)", n_refs, n_gal);
    if (encode_tensor < 1 || encode_tensor >= (int)e->tens.size()) return fail(XFR_INVALID_ARG, "bad tensor id");
    if (!e->weights_loaded) return fail(XFR_STATE_ERROR, "weights not loaded");
    hipStream_t s = (hipStream_t)stream;
    SweepCall call;
    rc = call.enter(e, s);
    if (rc != XFR_OK) return rc;
    ProbeSweep* sw = call.sw;
    StriseState* st = strise_state(e);
    const int B = e->max_batch, D = (int)e->tens[encode_tensor].per_n();
    const int nrg = n_refs + n_gal;
    rc = grow(&st->orig, &st->orig_cap, (size_t)2 * nrg);
    if (rc != XFR_OK) return rc;
    const long total = (long)n_masks + 1;
    const long rows = (total + B - 1) / B * B;
    // the whole sweep's cells and shifts go to the device once (6500 masks of 40 cells: 1 MB), on the side stream behind the caller's: the probe and
    // the fill may still be in flight there.  This is the sweep's one host wait
    rc = sweep_side_follows(sw, s);
    if (rc != XFR_OK) return rc;
    rc = upload_rows(st, cells_host, shifts_host, n_masks, g.n_elem, 0, rows, true, sw->s_gen);
    if (rc != XFR_OK) return rc;
    const int* cells_d = st->tab;
    const int* shifts_d = st->tab + (size_t)rows * g.n_elem;
    double* orig = st->orig;
    double* ginv = st->orig + nrg;
    rc = run_sweep(e, sw, total, encode_tensor, s,
        [&](long i, float* x, hipStream_t side) {
            launch_strise_masked(probe_u8_dev, fill_dev, cells_d + (size_t)i * B * g.n_elem, shifts_d + (size_t)i * B * 2, B, x, g, e->u8_pre.mean, side);
        },
        [&](long i, const float* emb, hipStream_t) {
            if (i == 0) launch_strise_orig(emb, refs_dev, n_refs, gallery_dev, n_gal, D, orig, ginv, s);      // image 0: the unmasked probe
            // images [i B, i B + B) of the list; image 0 is the probe, images beyond n_masks are padding
            const long lo = std::max(1L, i * B), hi = std::min(total, (i + 1) * B);
            launch_strise_score(emb, (int)(lo - i * B), (int)(hi - lo), refs_dev, n_refs, gallery_dev, n_gal, D, orig, ginv, scores_dev + (lo - 1), s);
        });
    if (rc != XFR_OK) return rc;
    if (orig_dev) HIP_TRY(hipMemcpyAsync(orig_dev, orig, nrg * sizeof(double), hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipGetLastError());
    return XFR_OK;
}

xfr_status xfr_strise_combine(xfr_engine* e, const double* weights_dev, int32_t n_selected, const int32_t* cells_host, const int32_t* shifts_host,
                              int32_t n_masks, const xfr_strise_geometry* geom, int32_t sign, double* sal_dev, void* stream)
{
    StriseGeom g;
    xfr_status rc = check_masks(e, cells_host, shifts_host, n_masks, geom, &g);
    if (rc != XFR_OK) return rc;
    if (!weights_dev || !sal_dev) return fail(XFR_INVALID_ARG, "strise: null argument");
    if (n_selected < 1 || n_selected > n_masks) return fail(XFR_INVALID_ARG, "strise: %d selected masks of %d", n_selected, n_masks);
    if (sign != 1 && sign != -1) return fail(XFR_INVALID_ARG, "strise: sign must be +1 or -1, got %d", sign);
    const int nc = g.gh * g.gw, ng = g.scale * g.scale;
    // layout of the table: cells [n_masks][n_elem], order [n_masks], group_off [ng + 1]
    std::vector<int> tab((size_t)n_masks * g.n_elem + n_masks + ng + 1);
    memcpy(tab.data(), cells_host, sizeof(int) * (size_t)n_masks * g.n_elem);
    {
        std::vector<int> seen(nc, -1);
        for (int k = 0; k < n_masks; ++k)
            for (int i = 0; i < g.n_elem; ++i) {
                const int c = cells_host[(size_t)k * g.n_elem + i];
                if (seen[c] == k) return fail(XFR_INVALID_ARG, "strise: mask %d draws cell %d twice", k, c);
                seen[c] = k;
            }
    }
    int* order = tab.data() + (size_t)n_masks * g.n_elem;
    int* off = order + n_masks;
    std::fill(off, off + ng + 1, 0);
    for (int k = 0; k < n_masks; ++k) off[shifts_host[2 * k] * g.scale + shifts_host[2 * k + 1] + 1] += 1;
    for (int q = 0; q < ng; ++q) off[q + 1] += off[q];
    {
        std::vector<int> at(off, off + ng);
        for (int k = 0; k < n_masks; ++k) order[at[shifts_host[2 * k] * g.scale + shifts_host[2 * k + 1]]++] = k;      // index order inside a group
    }
    hipStream_t s = (hipStream_t)stream;
    SweepCall call;      // the table may still be read by the side stream of an earlier xfr_strise_score: this call starts behind it
    rc = call.enter(e, s);
    if (rc != XFR_OK) return rc;
    StriseState* st = strise_state(e);
    rc = grow(&st->merge_ws, &st->merge_cap, (size_t)ng * nc + ng);
    if (rc != XFR_OK) return rc;
    rc = upload_table(st, tab, s);
    if (rc != XFR_OK) return rc;
    const int* order_d = st->tab + (size_t)n_masks * g.n_elem;
    launch_strise_merge(weights_dev, st->tab, order_d, order_d + n_masks, st->merge_ws, st->merge_ws + (size_t)ng * nc, (double)n_selected, (double)sign,
                        sal_dev, g, s);
    HIP_TRY(hipGetLastError());
    return XFR_OK;
}

xfr_status xfr_strise_debug_masks(xfr_engine* e, const int32_t* cells_host, const int32_t* shifts_host, int32_t n_masks, const xfr_strise_geometry* geom,
                                  int32_t first, int32_t count, double* masks_dev, void* stream)
{
    StriseGeom g;
    xfr_status rc = check_masks(e, cells_host, shifts_host, n_masks, geom, &g);
    if (rc != XFR_OK) return rc;
    if (!masks_dev) return fail(XFR_INVALID_ARG, "strise: null argument");
    if (first < 0 || count < 1 || (long)first + count > n_masks) return fail(XFR_INVALID_ARG, "strise: masks [%d, %d + %d) of %d", first, first, count, n_masks);
    hipStream_t s = (hipStream_t)stream;
    SweepCall call;
    rc = call.enter(e, s);
    if (rc != XFR_OK) return rc;
    StriseState* st = strise_state(e);
    rc = upload_rows(st, cells_host, shifts_host, n_masks, g.n_elem, first, count, false, s);
    if (rc != XFR_OK) return rc;
    launch_strise_masks(st->tab, st->tab + (size_t)count * g.n_elem, count, masks_dev, g, s);
    HIP_TRY(hipGetLastError());
    return XFR_OK;
}

xfr_status xfr_strise_debug_masked_probes(xfr_engine* e, const uint8_t* probe_u8_dev, const double* fill_dev, const int32_t* cells_host,
                                          const int32_t* shifts_host, int32_t n_masks, const xfr_strise_geometry* geom, int32_t first, int32_t count,
                                          float* out_nchw_dev, void* stream)
{
    StriseGeom g;
    xfr_status rc = check_masks(e, cells_host, shifts_host, n_masks, geom, &g);
    if (rc != XFR_OK) return rc;
    if (!probe_u8_dev || !fill_dev || !out_nchw_dev) return fail(XFR_INVALID_ARG, "strise: null argument");
    rc = check_u8(e);
    if (rc != XFR_OK) return rc;
    if (first < 0 || count < 1 || (long)first + count > n_masks || count > e->max_batch)
        return fail(XFR_INVALID_ARG, "strise: masks [%d, %d + %d) of %d, at most %d per call", first, first, count, n_masks, e->max_batch);
    hipStream_t s = (hipStream_t)stream;
    SweepCall call;
    rc = call.enter(e, s);
    if (rc != XFR_OK) return rc;
    StriseState* st = strise_state(e);
    rc = upload_rows(st, cells_host, shifts_host, n_masks, g.n_elem, first, count, false, s);
    if (rc != XFR_OK) return rc;
    launch_strise_masked(probe_u8_dev, fill_dev, st->tab, st->tab + (size_t)count * g.n_elem, count, out_nchw_dev, g, e->u8_pre.mean, s);
    HIP_TRY(hipGetLastError());
    return XFR_OK;
}

}  // extern "C"
