// strise_abi.hip -- the C ABI of STRise blackbox saliency (include/xfr_amd.h: xfr_strise_*; python/xfr/models/blackbox.py:299-442): argument checks,
// the two ends of the batched sweep (probe_sweep.hip), the grouping of the masks by shift for the merge.  The kernels are strise.hip.
#include "engine_internal.h"

namespace xfr {

// one tap table of Pillow's 8-bit resampling against the axis of n pixels it reads; `who` names the calling family in the text
xfr_status check_taps(const xfr_strise_tap* tab, int entries, int n, const char* what, const char* who)
{
    for (int i = 0; i < entries; ++i) {
        const xfr_strise_tap& t = tab[i];
        if (t.count < 1 || t.count > XFR_STRISE_MAX_TAPS)
            return fail(XFR_INVALID_ARG, "%s: %s table entry %d has count %d, outside [1, %d]", who, what, i, t.count, XFR_STRISE_MAX_TAPS);
        if (t.first < 0 || (long)t.first + t.count > n)
            return fail(XFR_INVALID_ARG, "%s: %s table entry %d reads [%d, %d + %d), a window outside the probe's %d", who, what, i, t.first, t.first, t.count, n);
        long sum = 0;
        for (int j = 0; j < t.count; ++j) {
            if (t.coef[j] < 0) return fail(XFR_INVALID_ARG, "%s: %s table entry %d has the negative coefficient %d", who, what, i, t.coef[j]);
            sum += t.coef[j];
        }
        if (sum * 255 + (1L << 21) > 2147483647L)
            return fail(XFR_INVALID_ARG, "%s: %s table entry %d: 255 x the coefficient sum %ld overflows int32", who, what, i, sum);
    }
    return XFR_OK;
}

}  // namespace xfr

namespace {

StriseState* strise_state(xfr_engine* e)
{
    if (!e->strise) e->strise.reset(new StriseState());
    return e->strise.get();
}

// the options of the _ex calls as the entry points use them; opt == NULL: the engine's input size, no quantisation
struct StriseOpt {
    int H = 0, W = 0;
    bool given = false, quant = false, lum = false;
    const xfr_strise_tap* row_tab = nullptr;
    const xfr_strise_tap* col_tab = nullptr;
    int rows_max = 0;                                  // luminance: the most probe rows one band of STRISE_LUM_BAND output rows reads
};

static_assert(sizeof(xfr_strise_tap) == sizeof(StriseTap) && XFR_STRISE_MAX_TAPS == STRISE_MAX_TAPS, "xfr_strise_tap is StriseTap");

// what every entry point checks before anything is launched
xfr_status check_masks(xfr_engine* e, const int32_t* cells, const int32_t* shifts, int n_masks, const xfr_strise_geometry* geom, const xfr_strise_options* opt,
                       StriseGeom* g, StriseOpt* o)
{
    if (!e) return fail(XFR_INVALID_ARG, "null engine");
    o->H = e->in_h;
    o->W = e->in_w;
    if (opt) {
        if (opt->struct_size != (int32_t)sizeof(xfr_strise_options))
            return fail(XFR_INVALID_ARG, "strise: options of struct_size %d, this library's xfr_strise_options has %d bytes", opt->struct_size,
                        (int)sizeof(xfr_strise_options));
        if (opt->probe_h < 1 || opt->probe_w < 1) return fail(XFR_INVALID_ARG, "strise: a probe of %d x %d", opt->probe_h, opt->probe_w);
        if (opt->quantize != 0 && opt->quantize != 1) return fail(XFR_INVALID_ARG, "strise: quantize must be 0 or 1, got %d", opt->quantize);
        o->given = true;
        o->H = opt->probe_h;
        o->W = opt->probe_w;
        o->quant = opt->quantize == 1;
        o->row_tab = opt->row_tab;
        o->col_tab = opt->col_tab;
    }
    if (!cells || !shifts || !geom) return fail(XFR_INVALID_ARG, "strise: null argument");
    if (n_masks < 1) return fail(XFR_INVALID_ARG, "strise: %d masks", n_masks);
    if (geom->grid_h < 1 || geom->grid_w < 1 || geom->mask_scale < 1 || geom->num_elements < 1)
        return fail(XFR_INVALID_ARG, "strise: grid %d x %d, mask_scale %d, %d elements per mask", geom->grid_h, geom->grid_w, geom->mask_scale, geom->num_elements);
    // a shift lies inside one cell of the image: a larger scale is no mask geometry, and scale^2 shift groups size the merge's workspace and grid
    if (geom->mask_scale > o->H || geom->mask_scale > o->W)
        return fail(XFR_INVALID_ARG, "strise: mask_scale %d exceeds the %d x %d input", geom->mask_scale, o->H, o->W);
    const long nc = (long)geom->grid_h * geom->grid_w;
    if (nc > STRISE_MAX_CELLS) return fail(XFR_INVALID_ARG, "strise: a grid of %d x %d cells exceeds %d", geom->grid_h, geom->grid_w, STRISE_MAX_CELLS);
    if (geom->num_elements > nc) return fail(XFR_INVALID_ARG, "strise: %d elements per mask in a grid of %ld cells", geom->num_elements, nc);
    for (long i = 0; i < (long)n_masks * geom->num_elements; ++i)
        if (cells[i] < 0 || cells[i] >= nc)
            return fail(XFR_INVALID_ARG, "strise: cell index %d of mask %ld outside the %d x %d grid", cells[i], i / geom->num_elements, geom->grid_h, geom->grid_w);
    for (long i = 0; i < 2L * n_masks; ++i)
        if (shifts[i] < 0 || shifts[i] >= geom->mask_scale)
            return fail(XFR_INVALID_ARG, "strise: shift %d of mask %ld outside [0, %d)", shifts[i], i / 2, geom->mask_scale);
    *g = StriseGeom{o->H, o->W, geom->grid_h, geom->grid_w, geom->mask_scale, geom->num_elements,
                    (double)geom->grid_h / (double)(o->H + geom->mask_scale), (double)geom->grid_w / (double)(o->W + geom->mask_scale)};
    return XFR_OK;
}

// what the network input needs of the engine.  quantize 0: only the arithmetic of convert_resnet101v4_image is built into the masked-probe kernel;
// quantize 1: the engine's own uint8 preprocessing, sub-mean at the probe's size or luminance behind the caller's resampling tables
xfr_status check_u8(xfr_engine* e, StriseOpt* o)
{
    if (o->quant && !e->u8_set)
        return fail(XFR_INVALID_ARG, "strise: quantize = 1 needs the engine's uint8 preprocessing (xfr_engine_set_u8_preprocess)");
    if (o->quant && e->u8_pre.kind == XFR_U8_LUMINANCE) {
        if (e->in_c != 1 || e->u8_pre.channels != 3)
            return fail(XFR_INVALID_ARG, "strise: XFR_U8_LUMINANCE of %d-channel images into a %d-channel network; 3 and 1 are built", e->u8_pre.channels, e->in_c);
        if (!o->row_tab || !o->col_tab)
            return fail(XFR_INVALID_ARG, "strise: an XFR_U8_LUMINANCE engine needs the resampling tables row_tab and col_tab");
        xfr_status rc = check_taps(o->row_tab, e->in_h, o->H, "row", "strise");
        if (rc != XFR_OK) return rc;
        rc = check_taps(o->col_tab, e->in_w, o->W, "column", "strise");
        if (rc != XFR_OK) return rc;
        for (int oy0 = 0; oy0 < e->in_h; oy0 += STRISE_LUM_BAND) {      // the kernel's own walk over a band
            int lo = o->H, hi = 0;
            for (int oy = oy0; oy < std::min(oy0 + STRISE_LUM_BAND, e->in_h); ++oy) {
                lo = std::min(lo, o->row_tab[oy].first);
                hi = std::max(hi, o->row_tab[oy].first + o->row_tab[oy].count);
            }
            o->rows_max = std::max(o->rows_max, hi - lo);
        }
        const size_t lds = strise_lum_lds_bytes(o->rows_max, o->W, e->in_w);
        if (lds > 60 * 1024)
            return fail(XFR_INVALID_ARG, "strise: a band of %d output rows reads %d probe rows of %d pixels: %zu bytes of LDS, more than %d", STRISE_LUM_BAND,
                        o->rows_max, o->W, lds, 60 * 1024);
        o->lum = true;
        return XFR_OK;
    }
    if (e->in_c != 3 || !e->u8_set || e->u8_pre.kind != XFR_U8_SUB_MEAN || e->u8_pre.channels != 3)
        return fail(XFR_INVALID_ARG, "strise: masked probes need a 3-channel network with XFR_U8_SUB_MEAN preprocessing of 3-channel images "
                                     "(xfr_engine_set_u8_preprocess); this engine takes %d channels", e->in_c);
    if (o->H != e->in_h || o->W != e->in_w)
        return fail(XFR_INVALID_ARG, "strise: a probe of %d x %d for an XFR_U8_SUB_MEAN engine whose input size is %d x %d", o->H, o->W, e->in_h, e->in_w);
    return XFR_OK;
}

// a host table into the state's `tab` on `s`; the host waits for the copy there: the table is pageable and local to the call
xfr_status upload_table(StriseState* st, const std::vector<int>& tab, hipStream_t s)
{
    xfr_status rc = st->tab.grow(tab.size());
    if (rc != XFR_OK) return rc;
    HIP_TRY(hipMemcpyAsync(st->tab, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    return XFR_OK;
}

constexpr int TAP_INTS = (int)(sizeof(StriseTap) / sizeof(int));

// rows [first, first + count) of the sweep's image list -- image 0 is the unmasked probe, images 1 .. n_masks the masks, anything beyond is padding
// -- as one table on the device: count x n_elem cells, then count x 2 shifts, then (luminance) the in_h + in_w resampling taps.  A row without a
// mask has cell -1 and shift 0, the all-ones mask of the closed-form law; under quantize = 1 its shift is -1: q = probe
xfr_status upload_rows(xfr_engine* e, StriseState* st, const int32_t* cells, const int32_t* shifts, int n_masks, int n_elem, long first, long count,
                       bool with_probe, const StriseOpt& o, hipStream_t s)
{
    const size_t taps = o.lum ? (size_t)(e->in_h + e->in_w) * TAP_INTS : 0;
    std::vector<int> tab((size_t)count * (n_elem + 2) + taps, -1);
    int* sh = tab.data() + (size_t)count * n_elem;
    for (long r = 0; r < count; ++r) {
        const long k = first + r - (with_probe ? 1 : 0);
        if (k >= 0 && k < n_masks) {
            memcpy(tab.data() + (size_t)r * n_elem, cells + (size_t)k * n_elem, sizeof(int) * n_elem);
            sh[2 * r] = shifts[2 * k];
            sh[2 * r + 1] = shifts[2 * k + 1];
        } else {
            sh[2 * r] = sh[2 * r + 1] = o.quant ? -1 : 0;
        }
    }
    if (o.lum) {
        int* t = sh + 2 * count;
        memcpy(t, o.row_tab, sizeof(StriseTap) * e->in_h);
        memcpy(t + (size_t)e->in_h * TAP_INTS, o.col_tab, sizeof(StriseTap) * e->in_w);
    }
    return upload_table(st, tab, s);
}

// the network input of `n` rows of an uploaded table (upload_rows) into x: the sweep's generate step and the parity hook
void launch_generate(xfr_engine* e, const uint8_t* probe, const double* fill, const int* tab, long rows, long row0, int n, float* x, const StriseGeom& g,
                     const StriseOpt& o, hipStream_t s)
{
    const int* cells = tab + (size_t)row0 * g.n_elem;
    const int* shifts = tab + (size_t)rows * g.n_elem + (size_t)row0 * 2;
    if (!o.quant) {
        launch_strise_masked(probe, fill, cells, shifts, n, x, g, e->u8_pre.mean, s);
    } else if (!o.lum) {
        launch_strise_quant(probe, fill, cells, shifts, n, x, g, e->u8_pre.mean, s);
    } else {
        const StriseTap* row_tab = reinterpret_cast<const StriseTap*>(tab + (size_t)rows * (g.n_elem + 2));
        launch_strise_quant_lum(probe, fill, cells, shifts, n, row_tab, row_tab + e->in_h, x, g, e->in_h, e->in_w, o.rows_max, e->u8_pre.weight, s);
    }
}

// masks [first, first + count) of the parity hooks; with options the range is one of the sweep's image list: first == -1 is image zero, the
// unmasked probe, and up to `pad` rows behind the last mask are the padding of the last batch
xfr_status check_range(const StriseOpt& o, int first, int count, int n_masks, int at_most, int pad)
{
    if (first < (o.given ? -1 : 0) || count < 1 || (long)first + count > (long)n_masks + (o.given ? pad : 0) || count > at_most)
        return fail(XFR_INVALID_ARG, "strise: masks [%d, %d + %d) of %d, at most %d per call", first, first, count, n_masks, at_most);
    return XFR_OK;
}

// What every entry point opens and closes with.  check(): the refusals in their order -- the masks and the options, the entry point's own pointers
// (args_ok), then (u8) what the network input needs of the engine.  The entry point's further checks follow it, then begin(): the sweep's guard on
// the caller's stream and the state; with a range, rows [first, first + count) of the image list as a table on the device (upload_rows).
struct Call : SweepCall {
    StriseGeom g;
    StriseOpt o;
    StriseState* st = nullptr;

    xfr_status check(xfr_engine* e, const int32_t* cells, const int32_t* shifts, int n_masks, const xfr_strise_geometry* geom,
                     const xfr_strise_options* opt, bool args_ok, bool u8)
    {
        const xfr_status rc = check_masks(e, cells, shifts, n_masks, geom, opt, &g, &o);
        if (rc != XFR_OK) return rc;
        if (!args_ok) return fail(XFR_INVALID_ARG, "strise: null argument");
        return u8 ? check_u8(e, &o) : XFR_OK;
    }

    xfr_status begin(xfr_engine* e, void* stream)
    {
        const xfr_status rc = enter(e, (hipStream_t)stream);
        if (rc == XFR_OK) st = strise_state(e);
        return rc;
    }

    xfr_status begin(xfr_engine* e, void* stream, const int32_t* cells, const int32_t* shifts, int n_masks, long first, long count, const StriseOpt& rows)
    {
        const xfr_status rc = begin(e, stream);
        return rc != XFR_OK ? rc : upload_rows(e, st, cells, shifts, n_masks, g.n_elem, first, count, false, rows, s);
    }

    static xfr_status finish() { HIP_TRY(hipGetLastError()); return XFR_OK; }
};

}  // namespace

extern "C" {

xfr_status xfr_strise_score_ex(xfr_engine* e, const uint8_t* probe_u8_dev, const double* fill_dev, const int32_t* cells_host, const int32_t* shifts_host,
                               int32_t n_masks, const xfr_strise_geometry* geom, const float* refs_dev, int32_t n_refs, const float* gallery_dev,
                               int32_t n_gal, int32_t encode_tensor, double* scores_dev, double* orig_dev, const xfr_strise_options* opt, void* stream)
{
    Call c;
    xfr_status rc = c.check(e, cells_host, shifts_host, n_masks, geom, opt, probe_u8_dev && fill_dev && refs_dev && gallery_dev && scores_dev, true);
    if (rc != XFR_OK) return rc;
    if (n_refs < 1 || n_gal < 1 || (n_refs != n_gal && n_refs != 1 && n_gal != 1))
        return fail(XFR_INVALID_ARG, "strise: %d references against %d gallery images do not broadcast (equal counts, or one of them 1)", n_refs, n_gal);
    if (encode_tensor < 1 || encode_tensor >= (int)e->tens.size()) return fail(XFR_INVALID_ARG, "bad tensor id");
    if (!e->weights_loaded) return fail(XFR_STATE_ERROR, "weights not loaded");
    rc = c.begin(e, stream);
    if (rc != XFR_OK) return rc;
    hipStream_t s = c.s;
    ProbeSweep* sw = c.sw;
    StriseState* st = c.st;
    const StriseGeom& g = c.g;
    const StriseOpt& o = c.o;
    const int B = e->max_batch, D = (int)e->tens[encode_tensor].per_n();
    const int nrg = n_refs + n_gal;
    rc = st->orig.grow((size_t)2 * nrg);
    if (rc != XFR_OK) return rc;
    const long total = (long)n_masks + 1;
    const long rows = (total + B - 1) / B * B;
    // the whole sweep's cells and shifts go to the device once (6500 masks of 40 cells: 1 MB), on the side stream behind the caller's: the probe and
    // the fill may still be in flight there.  This is the sweep's one host wait
    rc = sweep_side_follows(sw, s);
    if (rc != XFR_OK) return rc;
    rc = upload_rows(e, st, cells_host, shifts_host, n_masks, g.n_elem, 0, rows, true, o, sw->s_gen);
    if (rc != XFR_OK) return rc;
    const int* tab_d = st->tab;
    double* orig = st->orig;
    double* ginv = st->orig + nrg;
    rc = run_sweep(e, sw, total, encode_tensor, s,
        [&](long i, float* x, hipStream_t side) { launch_generate(e, probe_u8_dev, fill_dev, tab_d, rows, i * B, B, x, g, o, side); },
        [&](long i, const float* emb, hipStream_t) {
            if (i == 0) launch_strise_orig(emb, refs_dev, n_refs, gallery_dev, n_gal, D, orig, ginv, s);      // image 0: the unmasked probe
            // images [i B, i B + B) of the list; image 0 is the probe, images beyond n_masks are padding
            const long lo = std::max(1L, i * B), hi = std::min(total, (i + 1) * B);
            launch_strise_score(emb, (int)(lo - i * B), (int)(hi - lo), refs_dev, n_refs, gallery_dev, n_gal, D, orig, ginv, scores_dev + (lo - 1), s);
        });
    if (rc != XFR_OK) return rc;
    if (orig_dev) HIP_TRY(hipMemcpyAsync(orig_dev, orig, nrg * sizeof(double), hipMemcpyDeviceToDevice, s));
    return c.finish();
}

xfr_status xfr_strise_score(xfr_engine* e, const uint8_t* probe_u8_dev, const double* fill_dev, const int32_t* cells_host, const int32_t* shifts_host,
                            int32_t n_masks, const xfr_strise_geometry* geom, const float* refs_dev, int32_t n_refs, const float* gallery_dev,
                            int32_t n_gal, int32_t encode_tensor, double* scores_dev, double* orig_dev, void* stream)
{
    return xfr_strise_score_ex(e, probe_u8_dev, fill_dev, cells_host, shifts_host, n_masks, geom, refs_dev, n_refs, gallery_dev, n_gal, encode_tensor,
                               scores_dev, orig_dev, nullptr, stream);
}

xfr_status xfr_strise_combine_ex(xfr_engine* e, const double* weights_dev, int32_t n_selected, const int32_t* cells_host, const int32_t* shifts_host,
                                 int32_t n_masks, const xfr_strise_geometry* geom, int32_t sign, double* sal_dev, const xfr_strise_options* opt, void* stream)
{
    Call c;
    xfr_status rc = c.check(e, cells_host, shifts_host, n_masks, geom, opt, weights_dev && sal_dev, false);
    if (rc != XFR_OK) return rc;
    const StriseGeom& g = c.g;
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
    rc = c.begin(e, stream);      // the table may still be read by the side stream of an earlier xfr_strise_score: this call starts behind it
    if (rc != XFR_OK) return rc;
    StriseState* st = c.st;
    rc = st->merge_ws.grow((size_t)ng * nc + ng);
    if (rc == XFR_OK) rc = upload_table(st, tab, c.s);
    if (rc != XFR_OK) return rc;
    const int* order_d = st->tab + (size_t)n_masks * g.n_elem;
    launch_strise_merge(weights_dev, st->tab, order_d, order_d + n_masks, st->merge_ws, st->merge_ws + (size_t)ng * nc, (double)n_selected, (double)sign,
                        sal_dev, g, c.s);
    return c.finish();
}

xfr_status xfr_strise_combine(xfr_engine* e, const double* weights_dev, int32_t n_selected, const int32_t* cells_host, const int32_t* shifts_host,
                              int32_t n_masks, const xfr_strise_geometry* geom, int32_t sign, double* sal_dev, void* stream)
{
    return xfr_strise_combine_ex(e, weights_dev, n_selected, cells_host, shifts_host, n_masks, geom, sign, sal_dev, nullptr, stream);
}

xfr_status xfr_strise_debug_masks_ex(xfr_engine* e, const int32_t* cells_host, const int32_t* shifts_host, int32_t n_masks, const xfr_strise_geometry* geom,
                                     int32_t first, int32_t count, int32_t exact, double* masks_dev, const xfr_strise_options* opt, void* stream)
{
    Call c;
    xfr_status rc = c.check(e, cells_host, shifts_host, n_masks, geom, opt, masks_dev, false);
    if (rc != XFR_OK) return rc;
    if (exact != 0 && exact != 1) return fail(XFR_INVALID_ARG, "strise: exact must be 0 or 1, got %d", exact);
    if (first < 0 || count < 1 || (long)first + count > n_masks) return fail(XFR_INVALID_ARG, "strise: masks [%d, %d + %d) of %d", first, first, count, n_masks);
    rc = c.begin(e, stream, cells_host, shifts_host, n_masks, first, count, StriseOpt());
    if (rc != XFR_OK) return rc;
    launch_strise_masks(c.st->tab, c.st->tab + (size_t)count * c.g.n_elem, count, exact == 1, masks_dev, c.g, c.s);
    return c.finish();
}

xfr_status xfr_strise_debug_masks(xfr_engine* e, const int32_t* cells_host, const int32_t* shifts_host, int32_t n_masks, const xfr_strise_geometry* geom,
                                  int32_t first, int32_t count, double* masks_dev, void* stream)
{
    return xfr_strise_debug_masks_ex(e, cells_host, shifts_host, n_masks, geom, first, count, 0, masks_dev, nullptr, stream);
}

xfr_status xfr_strise_debug_masked_probes_ex(xfr_engine* e, const uint8_t* probe_u8_dev, const double* fill_dev, const int32_t* cells_host,
                                             const int32_t* shifts_host, int32_t n_masks, const xfr_strise_geometry* geom, int32_t first, int32_t count,
                                             float* out_dev, const xfr_strise_options* opt, void* stream)
{
    Call c;
    xfr_status rc = c.check(e, cells_host, shifts_host, n_masks, geom, opt, probe_u8_dev && fill_dev && out_dev, true);
    if (rc == XFR_OK) rc = check_range(c.o, first, count, n_masks, e->max_batch, e->max_batch);
    if (rc == XFR_OK) rc = c.begin(e, stream, cells_host, shifts_host, n_masks, first, count, c.o);
    if (rc != XFR_OK) return rc;
    launch_generate(e, probe_u8_dev, fill_dev, c.st->tab, count, 0, count, out_dev, c.g, c.o, c.s);
    return c.finish();
}

xfr_status xfr_strise_debug_masked_probes(xfr_engine* e, const uint8_t* probe_u8_dev, const double* fill_dev, const int32_t* cells_host,
                                          const int32_t* shifts_host, int32_t n_masks, const xfr_strise_geometry* geom, int32_t first, int32_t count,
                                          float* out_nchw_dev, void* stream)
{
    return xfr_strise_debug_masked_probes_ex(e, probe_u8_dev, fill_dev, cells_host, shifts_host, n_masks, geom, first, count, out_nchw_dev, nullptr, stream);
}

xfr_status xfr_strise_debug_quantized(xfr_engine* e, const uint8_t* probe_u8_dev, const double* fill_dev, const int32_t* cells_host,
                                      const int32_t* shifts_host, int32_t n_masks, const xfr_strise_geometry* geom, int32_t first, int32_t count,
                                      uint8_t* q_dev, const xfr_strise_options* opt, void* stream)
{
    if (e && !opt) return fail(XFR_INVALID_ARG, "strise: xfr_strise_debug_quantized needs options (the probe's size)");
    Call c;
    xfr_status rc = c.check(e, cells_host, shifts_host, n_masks, geom, opt, probe_u8_dev && fill_dev && q_dev, false);
    if (rc == XFR_OK) rc = check_range(c.o, first, count, n_masks, n_masks + 1 + e->max_batch, e->max_batch);
    StriseOpt q;
    q.quant = true;      // rows without a mask: q = probe
    if (rc == XFR_OK) rc = c.begin(e, stream, cells_host, shifts_host, n_masks, first, count, q);
    if (rc != XFR_OK) return rc;
    launch_strise_quant_u8(probe_u8_dev, fill_dev, c.st->tab, c.st->tab + (size_t)count * c.g.n_elem, count, q_dev, c.g, c.s);
    return c.finish();
}

}  // extern "C"
