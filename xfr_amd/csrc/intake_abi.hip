// intake_abi.hip -- the C ABI of image intake (include/xfr_amd.h: xfr_intake_u8, xfr_intake_u8_host, xfr_intake_set_kernels): argument checks, the
// Gaussian weights, the chunks of the pre-filter's workspace, the table uploads, the staging of host sources and the launches on the caller's stream.
// The kernels are intake.hip.  The calls use the engine for its device, its copy stream and error reporting only: no weights.
#include <cmath>
#include <cstring>
#include "engine_internal.h"

namespace {

static_assert(INTAKE_MAX_DIM == XFR_INTAKE_MAX_DIM && INTAKE_MAX_ITEMS == XFR_INTAKE_MAX_ITEMS && INTAKE_MAX_RADIUS == XFR_INTAKE_MAX_RADIUS,
              "the header states the kernels' limits");
static_assert(INTAKE_HEAD_F64 == XFR_INTAKE_HEAD_F64 && INTAKE_HEAD_F32 == XFR_INTAKE_HEAD_F32, "the header states the kernels' heads");
static_assert(sizeof(StriseTap) == sizeof(xfr_strise_tap), "a tap table is uploaded as it stands");

constexpr size_t PLANE_DOUBLES = (size_t)32 << 20;     // a chunk's crops fill at most this much of a plane (256 MB), one crop alone whatever it needs

bool overlap(const void* a, size_t na, const void* b, size_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

// scipy.ndimage.zoom sizes its own output, round(in * zoom) with zoom = 1 / (in / out); resize_linear pads or crops when that is not `out`
bool zoom_keeps_size(int in, int out) { return std::llround((double)in * (1.0 / ((double)in / (double)out))) == (long long)out; }

// numpy's float64 sum of a contiguous array: eight running sums below 128 values, halves above
double numpy_sum(const double* a, int n)
{
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; ++i) res += a[i];
        return res;
    }
    if (n <= 128) {
        double r[8];
        for (int j = 0; j < 8; ++j) r[j] = a[j];
        int i = 8;
        for (; i < n - (n % 8); i += 8)
            for (int j = 0; j < 8; ++j) r[j] += a[i + j];
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res += a[i];
        return res;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    return numpy_sum(a, n2) + numpy_sum(a + n2, n - n2);
}

// sigma and radius of the pre-filter along an axis of `in` values resized to `out`: radius 0 = no pass (the axis does not shrink, or its kernel is
// the single weight 1)
void prefilter_of(int in, int out, double* sigma, int* radius)
{
    const double f = (double)in / (double)out;
    *sigma = 0.0;
    *radius = 0;
    if (!(f > 1.0)) return;
    const double sg = (f - 1.0) / 2.0;
    if (!(sg > 1e-15)) return;
    *sigma = sg;
    *radius = (int)(4.0 * sg + 0.5);
}

// scipy's _gaussian_kernel1d: exp(-0.5 / sigma^2 * x^2) over x = -r .. r, divided by numpy's sum; the caller's own kernel where one was stated for
// exactly this sigma (numpy's exp is not every libm's)
void kernel_of(const IntakeState* st, double sigma, int radius, double* w)
{
    for (const IntakeKernel& k : st->stated)
        if (k.sigma == sigma && k.radius == radius) {
            std::memcpy(w, k.w, sizeof(double) * (radius + 1));
            return;
        }
    double phi[2 * INTAKE_MAX_RADIUS + 1];
    const double scale = -0.5 / (sigma * sigma);
    for (int x = -radius; x <= radius; ++x) phi[x + radius] = std::exp(scale * (double)(x * x));
    const double sum = numpy_sum(phi, 2 * radius + 1);
    for (int i = 0; i <= radius; ++i) w[i] = phi[i] / sum;
}

// every refusal of the two calls that needs neither the device nor the source's address
xfr_status check_call(xfr_engine* e, const void* src, size_t src_bytes, const xfr_intake_item* items, int n, int out_h, int out_w, const xfr_strise_tap* row_tab,
                      const xfr_strise_tap* col_tab, int final_h, int final_w, const void* out)
{
    if (!e) return fail(XFR_INVALID_ARG, "null engine");
    if (!src || !items || !out) return fail(XFR_INVALID_ARG, "intake_u8: null source, items or output");
    if (n < 1 || n > INTAKE_MAX_ITEMS) return fail(XFR_INVALID_ARG, "intake_u8: %d items, 1 to %d (XFR_INTAKE_MAX_ITEMS)", n, INTAKE_MAX_ITEMS);
    if (out_h < 1 || out_w < 1 || out_h > INTAKE_MAX_DIM || out_w > INTAKE_MAX_DIM)
        return fail(XFR_INVALID_ARG, "intake_u8: an output of %d x %d, every axis 1 to %d (XFR_INTAKE_MAX_DIM)", out_h, out_w, INTAKE_MAX_DIM);
    if ((row_tab == nullptr) != (col_tab == nullptr)) return fail(XFR_INVALID_ARG, "intake_u8: one tap table without the other (row_tab, col_tab)");
    if (row_tab) {
        if (final_h < 1 || final_w < 1 || final_h > INTAKE_MAX_DIM || final_w > INTAKE_MAX_DIM)
            return fail(XFR_INVALID_ARG, "intake_u8: a final size of %d x %d, every axis 1 to %d (XFR_INTAKE_MAX_DIM)", final_h, final_w, INTAKE_MAX_DIM);
        xfr_status rc = check_taps(row_tab, final_h, out_h, "row", "intake_u8");
        if (rc != XFR_OK) return rc;
        rc = check_taps(col_tab, final_w, out_w, "column", "intake_u8");
        if (rc != XFR_OK) return rc;
    }
    for (int i = 0; i < n; ++i) {
        const xfr_intake_item& it = items[i];
        if (it.channels != 1 && it.channels != 3 && it.channels != 4)
            return fail(XFR_INVALID_ARG, "intake_u8: item %d has %d channels; 1, 3 and 4 are built", i, it.channels);
        if (it.head != XFR_INTAKE_HEAD_F64 && it.head != XFR_INTAKE_HEAD_F32)
            return fail(XFR_INVALID_ARG, "intake_u8: item %d has head %d; XFR_INTAKE_HEAD_F64 (0) and XFR_INTAKE_HEAD_F32 (1) are built", i, it.head);
        if (it.h < 1 || it.w < 1 || it.h > INTAKE_MAX_DIM || it.w > INTAKE_MAX_DIM)
            return fail(XFR_INVALID_ARG, "intake_u8: item %d is %d x %d, every axis 1 to %d (XFR_INTAKE_MAX_DIM)", i, it.h, it.w, INTAKE_MAX_DIM);
        const int64_t row = (int64_t)it.w * it.channels;
        if (it.row_stride < row)
            return fail(XFR_INVALID_ARG, "intake_u8: item %d has a row stride of %d bytes, its rows hold %lld", i, it.row_stride, (long long)row);
        const int64_t last = it.offset + (int64_t)(it.h - 1) * it.row_stride + row;
        if (it.offset < 0 || (uint64_t)last > (uint64_t)src_bytes)
            return fail(XFR_INVALID_ARG, "intake_u8: item %d reads bytes [%lld, %lld), the source holds %zu", i, (long long)it.offset, (long long)last, src_bytes);
        if (it.h == out_h && it.w == out_w) continue;
        double sg;
        int r;
        prefilter_of(it.h, out_h, &sg, &r);
        if (r <= INTAKE_MAX_RADIUS) prefilter_of(it.w, out_w, &sg, &r);
        if (r > INTAKE_MAX_RADIUS)
            return fail(XFR_INVALID_ARG, "intake_u8: item %d, %d x %d to %d x %d, needs a pre-filter of radius %d, at most %d (XFR_INTAKE_MAX_RADIUS)", i, it.h, it.w,
                        out_h, out_w, r, INTAKE_MAX_RADIUS);
        if (!zoom_keeps_size(it.h, out_h) || !zoom_keeps_size(it.w, out_w))
            return fail(XFR_INVALID_ARG, "intake_u8: item %d, %d x %d to %d x %d, is a size the zoom rounds away from (the padded result stays on the host)", i, it.h,
                        it.w, out_h, out_w);
    }
    return XFR_OK;
}

IntakeState* state_of(xfr_engine* e)
{
    if (!e->intake) e->intake.reset(new IntakeState());
    return e->intake.get();
}

// the checked call on sources that are on the device
xfr_status run(xfr_engine* e, const uint8_t* src_dev, const xfr_intake_item* items, int n, int H, int W, const xfr_strise_tap* row_tab,
               const xfr_strise_tap* col_tab, int fh, int fw, uint8_t* out_dev, hipStream_t s)
{
    IntakeState* st = state_of(e);
    if (!st->ev_done) XFR_TRY(st->ev_done.create());
    if (st->done_recorded) HIP_TRY(hipStreamWaitEvent(s, st->ev_done, 0));

    // the crops as the kernels see them, their weights, and the chunks: consecutive crops whose planes fit PLANE_DOUBLES
    std::vector<IntakeItem> dev((size_t)n);
    std::vector<double> wts;
    std::vector<int> chunk_first(1, 0);
    size_t used = 0, need_a = 0, need_b = 0;
    bool any_filter = false;
    for (int i = 0; i < n; ++i) {
        const xfr_intake_item& it = items[i];
        IntakeItem& d = dev[i];
        d = IntakeItem{};
        d.src = (long)it.offset;
        d.h = it.h; d.w = it.w; d.stride = it.row_stride; d.C = it.channels; d.head = it.head;
        d.identity = it.h == H && it.w == W;
        d.sy = (double)it.h / (double)H;
        d.sx = (double)it.w / (double)W;
        d.zoom_from = INTAKE_FROM_U8;
        double sgy = 0.0, sgx = 0.0;
        if (!d.identity) { prefilter_of(it.h, H, &sgy, &d.ry); prefilter_of(it.w, W, &sgx, &d.rx); }
        const size_t elems = (d.ry > 0 || d.rx > 0) ? (size_t)it.h * it.w * it.channels : 0;
        if (elems) {
            if (!any_filter) { wts.assign((size_t)n * 2 * INTAKE_WEIGHTS, 0.0); any_filter = true; }
            if (d.ry > 0) kernel_of(st, sgy, d.ry, &wts[((size_t)i * 2) * INTAKE_WEIGHTS]);
            if (d.rx > 0) kernel_of(st, sgx, d.rx, &wts[((size_t)i * 2 + 1) * INTAKE_WEIGHTS]);
            d.zoom_from = (d.ry > 0 && d.rx > 0) ? INTAKE_FROM_B : INTAKE_FROM_A;
            if (used > 0 && used + elems > PLANE_DOUBLES) { chunk_first.push_back(i); used = 0; }
            d.ws = (long)used;
            used += elems;
            need_a = std::max(need_a, used);
            if (d.zoom_from == INTAKE_FROM_B) need_b = std::max(need_b, used);
        }
    }
    chunk_first.push_back(n);

    xfr_status rc = st->items.grow((size_t)n);
    if (rc == XFR_OK) rc = st->lohi.grow((size_t)n * 2);
    if (rc == XFR_OK && any_filter) rc = st->wts.grow(wts.size());
    if (rc == XFR_OK && need_a) rc = st->plane_a.grow(need_a);
    if (rc == XFR_OK && need_b) rc = st->plane_b.grow(need_b);
    if (rc == XFR_OK && row_tab) rc = st->q.grow((size_t)n * H * W * 3);
    if (rc == XFR_OK && row_tab) rc = st->mid.grow((size_t)n * H * fw * 3);
    if (rc == XFR_OK && row_tab) rc = st->taps.grow((size_t)fh + fw);
    if (rc != XFR_OK) return rc;
    HIP_TRY(hipMemcpyAsync(st->items, dev.data(), sizeof(IntakeItem) * n, hipMemcpyHostToDevice, s));
    if (any_filter) HIP_TRY(hipMemcpyAsync(st->wts, wts.data(), sizeof(double) * wts.size(), hipMemcpyHostToDevice, s));
    if (row_tab) {
        HIP_TRY(hipMemcpyAsync(st->taps, row_tab, sizeof(StriseTap) * fh, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(st->taps + fh, col_tab, sizeof(StriseTap) * fw, hipMemcpyHostToDevice, s));
    }
    HIP_TRY(hipStreamSynchronize(s));                  // the tables are pageable and local to the call

    uint8_t* bytes = row_tab ? st->q : out_dev;
    launch_intake_range(src_dev, st->items, n, st->lohi, s);
    for (size_t c = 0; c + 1 < chunk_first.size(); ++c) {
        const int i0 = chunk_first[c], cn = chunk_first[c + 1] - i0;
        long max_elems = 0;
        int which = 0;
        for (int i = i0; i < i0 + cn; ++i) {
            const IntakeItem& d = dev[i];
            if (d.ry > 0 || d.rx > 0) max_elems = std::max(max_elems, (long)d.h * d.w * d.C);
            which |= d.ry > 0 ? (d.rx > 0 ? 1 | 4 : 1) : (d.rx > 0 ? 2 : 0);
        }
        if (which)
            launch_intake_prefilter(src_dev, st->items + i0, cn, st->wts + (size_t)i0 * 2 * INTAKE_WEIGHTS, st->plane_a, st->plane_b, max_elems, which, s);
        launch_intake_zoom(src_dev, st->items + i0, cn, st->lohi + (size_t)i0 * 2, st->plane_a, st->plane_b, H, W, bytes + (size_t)i0 * H * W * 3, s);
    }
    if (row_tab) launch_intake_taps(st->q, n, H, W, st->taps, st->taps + fh, fh, fw, st->mid, out_dev, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(st->ev_done, s));
    st->done_recorded = true;
    return XFR_OK;
}

}  // namespace

extern "C" {

xfr_status xfr_intake_set_kernels(xfr_engine* e, const double* sigmas_host, const int32_t* radii_host, const double* weights_host, int32_t count)
{
    if (!e) return fail(XFR_INVALID_ARG, "null engine");
    if (count < 0 || (count > 0 && (!sigmas_host || !radii_host || !weights_host)))
        return fail(XFR_INVALID_ARG, "intake_set_kernels: %d kernels with a null array", count);
    for (int i = 0; i < count; ++i)
        if (!(sigmas_host[i] > 0.0) || radii_host[i] < 1 || radii_host[i] > INTAKE_MAX_RADIUS)
            return fail(XFR_INVALID_ARG, "intake_set_kernels: kernel %d has sigma %g and radius %d, sigma > 0 and a radius of 1 to %d (XFR_INTAKE_MAX_RADIUS)", i,
                        sigmas_host[i], radii_host[i], INTAKE_MAX_RADIUS);
    IntakeState* st = state_of(e);
    st->stated.resize((size_t)count);
    for (int i = 0; i < count; ++i) {
        st->stated[i].sigma = sigmas_host[i];
        st->stated[i].radius = radii_host[i];
        std::memcpy(st->stated[i].w, weights_host + (size_t)i * INTAKE_WEIGHTS, sizeof(double) * INTAKE_WEIGHTS);
    }
    return XFR_OK;
}

xfr_status xfr_intake_u8(xfr_engine* e, const uint8_t* src_dev, size_t src_bytes, const xfr_intake_item* items_host, int32_t n, int32_t out_h, int32_t out_w,
                         const xfr_strise_tap* row_tab, const xfr_strise_tap* col_tab, int32_t final_h, int32_t final_w, uint8_t* out_dev, void* stream)
{
    xfr_status rc = check_call(e, src_dev, src_bytes, items_host, n, out_h, out_w, row_tab, col_tab, final_h, final_w, out_dev);
    if (rc != XFR_OK) return rc;
    const size_t out_b = (size_t)n * (row_tab ? (size_t)final_h * final_w : (size_t)out_h * out_w) * 3;
    if (overlap(src_dev, src_bytes, out_dev, out_b)) return fail(XFR_INVALID_ARG, "intake_u8: the output overlaps the source");
    HIP_TRY(hipSetDevice(e->device));
    return run(e, src_dev, items_host, n, out_h, out_w, row_tab, col_tab, final_h, final_w, out_dev, (hipStream_t)stream);
}

xfr_status xfr_intake_u8_host(xfr_engine* e, const uint8_t* src_host, size_t src_bytes, const xfr_intake_item* items_host, int32_t n, int32_t out_h,
                              int32_t out_w, const xfr_strise_tap* row_tab, const xfr_strise_tap* col_tab, int32_t final_h, int32_t final_w, uint8_t* out_dev,
                              void* stream)
{
    xfr_status rc = check_call(e, src_host, src_bytes, items_host, n, out_h, out_w, row_tab, col_tab, final_h, final_w, out_dev);
    if (rc != XFR_OK) return rc;
    if (src_bytes == 0) return fail(XFR_INVALID_ARG, "intake_u8: an empty source");
    HIP_TRY(hipSetDevice(e->device));
    IntakeState* st = state_of(e);
    hipStream_t s = (hipStream_t)stream;
    if (!e->s_copy) XFR_TRY(e->s_copy.create());
    if (!st->ev_copied) XFR_TRY(st->ev_copied.create());
    if (st->copied_recorded) HIP_TRY(hipEventSynchronize(st->ev_copied));      // the pinned buffer is free again
    if (st->stage_host.cap < src_bytes) XFR_TRY(st->stage_host.alloc(src_bytes));
    rc = st->stage_dev.grow(src_bytes);
    if (rc != XFR_OK) return rc;
    std::memcpy(st->stage_host, src_host, src_bytes);
    if (st->done_recorded) HIP_TRY(hipStreamWaitEvent(e->s_copy, st->ev_done, 0));      // the previous call's kernels read the device copy
    HIP_TRY(hipMemcpyAsync(st->stage_dev, st->stage_host, src_bytes, hipMemcpyHostToDevice, e->s_copy));
    HIP_TRY(hipEventRecord(st->ev_copied, e->s_copy));
    st->copied_recorded = true;
    HIP_TRY(hipStreamWaitEvent(s, st->ev_copied, 0));
    return run(e, st->stage_dev, items_host, n, out_h, out_w, row_tab, col_tab, final_h, final_w, out_dev, s);
}

}  // extern "C"
