// match_abi.hip -- the C ABI of match calibration (include/xfr_amd.h: xfr_embed_templates, xfr_pair_dists, xfr_nearest_rows): argument checks,
// the upload of the caller's index tables, the launches on the caller's stream.  The kernels are match.hip.  The calls use the engine for its
// device and error reporting only: no weights, no workspace, and nothing of the probe sweep.
#include <vector>
#include "engine_internal.h"

namespace {

static_assert(MATCH_MAX_K == XFR_MATCH_MAX_K && MATCH_MAX_D == XFR_MATCH_MAX_D, "the header states the kernels' limits");

// do [a, a + na) and [b, b + nb) (bytes) share a byte?
bool overlap(const void* a, size_t na, const void* b, size_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

xfr_status check_dim(const char* what, int D)
{
    if (D < 1 || D > MATCH_MAX_D) return fail(XFR_INVALID_ARG, "%s: rows of %d values, 1 to %d (XFR_MATCH_MAX_D)", what, D, MATCH_MAX_D);
    return XFR_OK;
}

// the table on the device, behind the previous call's kernels; `s` holds it when this returns
xfr_status upload(xfr_engine* e, const std::vector<int>& tab, hipStream_t s, int** dev)
{
    HIP_TRY(hipSetDevice(e->device));
    if (!e->match) e->match.reset(new MatchState());
    MatchState* st = e->match.get();
    if (!st->ev_done) XFR_TRY(st->ev_done.create());
    if (st->done_recorded) HIP_TRY(hipStreamWaitEvent(s, st->ev_done, 0));
    const xfr_status rc = st->tab.grow(tab.size());
    if (rc != XFR_OK) return rc;
    HIP_TRY(hipMemcpyAsync(st->tab, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));                  // the host vector goes away with the call
    *dev = st->tab;
    return XFR_OK;
}

// what a call that launched closes with
xfr_status finish(xfr_engine* e, hipStream_t s, bool uses_tab)
{
    HIP_TRY(hipGetLastError());
    if (uses_tab) {
        HIP_TRY(hipEventRecord(e->match->ev_done, s));
        e->match->done_recorded = true;
    }
    return XFR_OK;
}

}  // namespace

extern "C" {

xfr_status xfr_embed_templates(xfr_engine* e, const float* emb_dev, int32_t n, int32_t d, const int32_t* rows_host, const int32_t* offsets_host,
                               int32_t n_groups, int32_t normalize_rows, float* out_dev, void* stream)
{
    if (!e) return fail(XFR_INVALID_ARG, "null engine");
    if (!emb_dev || !rows_host || !offsets_host || !out_dev) return fail(XFR_INVALID_ARG, "embed_templates: null argument");
    if (n < 1 || n_groups < 1) return fail(XFR_INVALID_ARG, "embed_templates: %d rows, %d groups", n, n_groups);
    xfr_status rc = check_dim("embed_templates", d);
    if (rc != XFR_OK) return rc;
    if (offsets_host[0] != 0) return fail(XFR_INVALID_ARG, "embed_templates: offsets start at %d, not 0", offsets_host[0]);
    for (int g = 0; g < n_groups; ++g)
        if (offsets_host[g + 1] <= offsets_host[g])
            return fail(XFR_INVALID_ARG, "embed_templates: group %d is [%d, %d), a group holds at least one row", g, offsets_host[g], offsets_host[g + 1]);
    const int total = offsets_host[n_groups];
    for (int p = 0; p < total; ++p)
        if (rows_host[p] < 0 || rows_host[p] >= n) return fail(XFR_INVALID_ARG, "embed_templates: row %d at place %d of the list, the matrix has %d", rows_host[p], p, n);
    if (overlap(emb_dev, (size_t)n * d * sizeof(float), out_dev, (size_t)n_groups * d * sizeof(float)))
        return fail(XFR_INVALID_ARG, "embed_templates: the templates overlap the embeddings");
    std::vector<int> tab(offsets_host, offsets_host + n_groups + 1);
    tab.insert(tab.end(), rows_host, rows_host + total);
    hipStream_t s = (hipStream_t)stream;
    int* tab_dev = nullptr;
    rc = upload(e, tab, s, &tab_dev);
    if (rc != XFR_OK) return rc;
    launch_embed_templates(emb_dev, d, tab_dev, n_groups, normalize_rows ? 1 : 0, out_dev, s);
    return finish(e, s, true);
}

xfr_status xfr_pair_dists(xfr_engine* e, const float* a_dev, int32_t na, const float* b_dev, int32_t nb, int32_t d, const int32_t* pairs_host,
                          int32_t n_pairs, float* out_dev, void* stream)
{
    if (!e) return fail(XFR_INVALID_ARG, "null engine");
    if (!a_dev || !b_dev || !pairs_host || !out_dev) return fail(XFR_INVALID_ARG, "pair_dists: null argument");
    if (na < 1 || nb < 1 || n_pairs < 1) return fail(XFR_INVALID_ARG, "pair_dists: %d and %d rows, %d pairs", na, nb, n_pairs);
    xfr_status rc = check_dim("pair_dists", d);
    if (rc != XFR_OK) return rc;
    for (int p = 0; p < n_pairs; ++p) {
        const int i = pairs_host[2 * p], j = pairs_host[2 * p + 1];
        if (i < 0 || i >= na || j < 0 || j >= nb) return fail(XFR_INVALID_ARG, "pair_dists: pair %d is (%d, %d), the matrices have %d and %d rows", p, i, j, na, nb);
    }
    const size_t out_bytes = (size_t)n_pairs * sizeof(float);
    if (overlap(a_dev, (size_t)na * d * sizeof(float), out_dev, out_bytes) || overlap(b_dev, (size_t)nb * d * sizeof(float), out_dev, out_bytes))
        return fail(XFR_INVALID_ARG, "pair_dists: the distances overlap a matrix");
    std::vector<int> tab(pairs_host, pairs_host + 2 * (size_t)n_pairs);
    hipStream_t s = (hipStream_t)stream;
    int* tab_dev = nullptr;
    rc = upload(e, tab, s, &tab_dev);
    if (rc != XFR_OK) return rc;
    launch_pair_dists(a_dev, b_dev, d, tab_dev, n_pairs, out_dev, s);
    return finish(e, s, true);
}

xfr_status xfr_nearest_rows(xfr_engine* e, const float* q_dev, int32_t nq, const float* g_dev, int32_t ng, int32_t d, int32_t k,
                            int32_t exclude_same_index, int32_t* idx_dev, float* dist_dev, void* stream)
{
    if (!e) return fail(XFR_INVALID_ARG, "null engine");
    if (!q_dev || !g_dev || !idx_dev || !dist_dev) return fail(XFR_INVALID_ARG, "nearest_rows: null argument");
    if (nq < 1 || ng < 1) return fail(XFR_INVALID_ARG, "nearest_rows: %d queries, %d gallery rows", nq, ng);
    const xfr_status rc = check_dim("nearest_rows", d);
    if (rc != XFR_OK) return rc;
    const int excl = exclude_same_index ? 1 : 0;
    if (k < 1 || k > MATCH_MAX_K) return fail(XFR_INVALID_ARG, "nearest_rows: k = %d, 1 to %d (XFR_MATCH_MAX_K)", k, MATCH_MAX_K);
    if (k > ng - excl)
        return fail(XFR_INVALID_ARG, "nearest_rows: k = %d of %d gallery rows%s", k, ng, excl ? ", one of which every query skips (exclude_same_index)" : "");
    const size_t qb = (size_t)nq * d * sizeof(float), gb = (size_t)ng * d * sizeof(float), ob = (size_t)nq * k * 4;
    if (overlap(q_dev, qb, idx_dev, ob) || overlap(q_dev, qb, dist_dev, ob) || overlap(g_dev, gb, idx_dev, ob) || overlap(g_dev, gb, dist_dev, ob) ||
        overlap(idx_dev, ob, dist_dev, ob))
        return fail(XFR_INVALID_ARG, "nearest_rows: the outputs overlap a matrix or one another");
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    launch_nearest_rows(q_dev, nq, g_dev, ng, d, k, excl, idx_dev, dist_dev, s);
    return finish(e, s, false);
}

}  // extern "C"
