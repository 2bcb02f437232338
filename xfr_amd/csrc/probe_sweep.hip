// probe_sweep.hip -- the batched sweep that STRise (strise_abi.hip) and inpainting-game scoring (inpaint_abi.hip) share: the images of batch i + 1 are
// built on a side stream into one of two input buffers while batch i runs through xfr_forward on the caller's stream and a small kernel consumes its
// embeddings.  One object per engine, so a call of either family starts behind the previous call of either family.  No kernels.
#include "engine_internal.h"

namespace xfr {

xfr_status sweep_enter(xfr_engine* e, hipStream_t s, ProbeSweep** out)
{
    HIP_TRY(hipSetDevice(e->device));
    if (!e->sweep) e->sweep.reset(new ProbeSweep());
    ProbeSweep* sw = e->sweep.get();
    if (!sw->s_gen) {
        Event in, done, ready[2], free_[2];
        Stream gen;
        XFR_TRY(in.create());
        XFR_TRY(done.create());
        for (int k = 0; k < 2; ++k) {
            XFR_TRY(ready[k].create());
            XFR_TRY(free_[k].create());
        }
        XFR_TRY(gen.create());
        sw->ev_in = std::move(in); sw->ev_done = std::move(done); sw->s_gen = std::move(gen);
        for (int k = 0; k < 2; ++k) { sw->ev_ready[k] = std::move(ready[k]); sw->ev_free[k] = std::move(free_[k]); }
    }
    // the engine's buffers may still be read by the side stream, or by the previous call on another stream: this call starts behind both
    HIP_TRY(hipEventRecord(sw->ev_in, sw->s_gen));
    HIP_TRY(hipStreamWaitEvent(s, sw->ev_in, 0));
    if (sw->done_recorded) HIP_TRY(hipStreamWaitEvent(s, sw->ev_done, 0));
    *out = sw;
    return XFR_OK;
}

void sweep_leave(ProbeSweep* sw, hipStream_t s)
{
    if (hipEventRecord(sw->ev_done, s) == hipSuccess) sw->done_recorded = true;      // no fail(): an error text of the call stays
}

xfr_status sweep_side_follows(ProbeSweep* sw, hipStream_t s)
{
    HIP_TRY(hipEventRecord(sw->ev_in, s));
    HIP_TRY(hipStreamWaitEvent(sw->s_gen, sw->ev_in, 0));
    return XFR_OK;
}

xfr_status run_sweep(xfr_engine* e, ProbeSweep* sw, long n_images, int encode_tensor, hipStream_t s, const SweepGenerate& generate,
                     const SweepConsume& consume)
{
    const int B = e->max_batch;
    for (int k = 0; k < 2; ++k)
        if (!sw->xbuf[k]) XFR_TRY(sw->xbuf[k].alloc((size_t)B * e->in_c * e->in_h * e->in_w));
    xfr_status rc = sw->emb.grow((size_t)B * e->tens[encode_tensor].per_n());
    if (rc != XFR_OK) return rc;
    const long n_batches = (n_images + B - 1) / B;      // the last one is padded: generate fills it, consume drops what lies beyond n_images
    bool used[2] = {false, false};
    auto gen = [&](long i) -> xfr_status {
        const int k = (int)(i & 1);
        if (used[k]) HIP_TRY(hipStreamWaitEvent(sw->s_gen, sw->ev_free[k], 0));      // the forward that last read this buffer
        generate(i, sw->xbuf[k], sw->s_gen);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(sw->ev_ready[k], sw->s_gen));
        return XFR_OK;
    };
    rc = gen(0);
    for (long i = 0; rc == XFR_OK && i < n_batches; ++i) {
        const int k = (int)(i & 1);
        if (i + 1 < n_batches) {
            rc = gen(i + 1);
            if (rc != XFR_OK) break;
        }
        hipError_t he = hipStreamWaitEvent(s, sw->ev_ready[k], 0);
        if (he != hipSuccess) { rc = fail(XFR_HIP_ERROR, "hipStreamWaitEvent failed: %s", hipGetErrorString(he)); break; }
        rc = xfr_forward(e, sw->xbuf[k], B, encode_tensor, sw->emb, s);
        if (rc != XFR_OK) break;
        he = hipEventRecord(sw->ev_free[k], s);
        if (he != hipSuccess) { rc = fail(XFR_HIP_ERROR, "hipEventRecord failed: %s", hipGetErrorString(he)); break; }
        used[k] = true;
        consume(i, sw->emb, s);
        he = hipGetLastError();
        if (he != hipSuccess) rc = fail(XFR_HIP_ERROR, "hipGetLastError() failed: %s", hipGetErrorString(he));
    }
    if (rc != XFR_OK) {
        // whatever happens, the caller's stream ends up ordered behind the side stream: nothing of this call outlives what the caller enqueues next
        const std::string why = g_err;
        if (hipEventRecord(sw->ev_in, sw->s_gen) == hipSuccess) (void)hipStreamWaitEvent(s, sw->ev_in, 0);
        g_err = why;
    }
    return rc;
}

}  // namespace xfr
