// subtree.hip -- the C ABI of the "next" rows: layerwise and weighted-subtree EBP (sweeps with priors, captures and stored firings) and their scratch.
#include "engine_internal.h"

extern "C" {

// ---- "next" rows: layerwise / weighted-subtree EBP -----------------------------------------------------------------------
static xfr_status ensure_subtree_scratch(xfr_engine* e)
{
    if (e->cap_dev) return XFR_OK;
    const size_t nf = e->trace_cap + 1, cap = nf * 2 * (size_t)e->max_batch;
    DevBuf<float> cap_dev, tab_val_d, stat_v, store_dev;
    DevBuf<int> tab_elem_d, stat_i, stat_f2u;
    PinnedBuf<int> tab_elem_h;
    PinnedBuf<float> tab_val_h;
    Event ev_tab;
    DevBuf<char> stat_scratch;
    DevBuf<StatDesc> stat_desc;
    XFR_TRY(cap_dev.alloc(cap));
    XFR_TRY(tab_elem_d.alloc(cap));
    XFR_TRY(tab_val_d.alloc(cap));
    XFR_TRY(tab_elem_h.alloc(cap));
    XFR_TRY(tab_val_h.alloc(cap));
    XFR_TRY(ev_tab.create());
    XFR_TRY(stat_v.alloc(nf * e->max_batch));
    XFR_TRY(stat_i.alloc(nf * e->max_batch));
    XFR_TRY(stat_scratch.alloc(subtree_stats_scratch_bytes(e->max_batch, (int)nf)));
    XFR_TRY(stat_desc.alloc(nf));
    XFR_TRY(stat_f2u.alloc(nf));
    XFR_TRY(store_dev.alloc(2 * (size_t)e->max_batch * e->max_per_n()));
    e->tab_cap = cap;
    e->cap_dev = std::move(cap_dev); e->tab_elem_d = std::move(tab_elem_d); e->tab_val_d = std::move(tab_val_d);
    e->tab_elem_h = std::move(tab_elem_h); e->tab_val_h = std::move(tab_val_h); e->ev_tab = std::move(ev_tab);
    e->stat_v = std::move(stat_v); e->stat_i = std::move(stat_i); e->stat_scratch = std::move(stat_scratch);
    e->stat_desc = std::move(stat_desc); e->stat_f2u = std::move(stat_f2u); e->store_dev = std::move(store_dev);
    return XFR_OK;
}

xfr_status xfr_subtree_weights(xfr_engine* e, const float* x_dev, int32_t n, int32_t seed_tensor, const float* seed_dev,
                               int32_t gate_ge0, float* w_host, int32_t* idx_host, int32_t capacity, void* stream)
{
    xfr_status st = check_run(e, x_dev, n);
    if (st != XFR_OK) return st;
    if (!seed_dev || !w_host || !idx_host) return fail(XFR_INVALID_ARG, "null argument");
    st = ensure_subtree_scratch(e);
    if (st != XFR_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    BwdPlan* plan = nullptr;
    st = get_plan(e, seed_tensor, &plan, true);
    if (st != XFR_OK) return st;
    const int nf = plan->n_firings;
    if (capacity < nf * n) return fail(XFR_INVALID_ARG, "need room for %d x %d values", nf, n);
    st = forward_all(e, x_dev, n, seed_tensor, false, s, true);       // no positive pass, but the MaxFeatureMap VJPs below read the raw halves
    if (st != XFR_OK) return st;
    const Tensor& sd = e->tens[seed_tensor];
    launch_seed_to_cnhw(seed_dev, e->G(seed_tensor), 2 * n, sd.C, sd.HW(), s);
    st = run_backward(e, SweepCtx(), *plan, n, 2, s);
    if (st != XFR_OK) return st;
    if (e->stat_plan != plan) {       // descriptor table of this plan: one entry per distinct gradient tensor
        std::vector<StatDesc> desc;
        std::vector<int> f2u(nf);
        int last_t = -1;
        for (int f = 0; f < nf; ++f) {
            const int t = plan->firing_tensor[f];
            if (t != last_t) desc.push_back(StatDesc{e->G(t), e->tens[t].C, e->tens[t].HW()});   // several hooks on one tensor see the same gradient
            f2u[f] = (int)desc.size() - 1;
            last_t = t;
        }
        HIP_TRY(hipMemcpyAsync(e->stat_desc, desc.data(), desc.size() * sizeof(StatDesc), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(e->stat_f2u, f2u.data(), f2u.size() * sizeof(int), hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));     // the host vectors go out of scope
        e->stat_plan = plan;
        e->stat_nu = (int)desc.size();
    }
    launch_subtree_stats(e->stat_desc, e->stat_nu, e->stat_f2u, nf, e->stat_v, e->stat_i, e->stat_scratch, n, gate_ge0, s);
    HIP_TRY(hipMemcpyAsync(w_host, e->stat_v, (size_t)nf * n * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(idx_host, e->stat_i, (size_t)nf * n * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return XFR_OK;
}

// stage the element / value tables of a call, whose sweep finds them through cx: the pinned host copies may only be rewritten once the previous
// call's host-to-device copy has completed
static xfr_status tables_begin(xfr_engine* e, SweepCtx& cx, int nf, int rows)
{
    if ((size_t)nf * rows > e->tab_cap) return fail(XFR_INVALID_ARG, "%d firings x %d gradient rows exceed the table scratch", nf, rows);
    HIP_TRY(hipEventSynchronize(e->ev_tab));
    cx.tab_sb = rows;
    cx.tab_elem = e->tab_elem_d; cx.tab_val = e->tab_val_d; cx.cap_dst = e->cap_dev;
    for (size_t i = 0; i < (size_t)nf * rows; ++i) { e->tab_elem_h[i] = -1; e->tab_val_h[i] = 0.f; }
    return XFR_OK;
}

static xfr_status tables_commit(xfr_engine* e, const SweepCtx& cx, int nf, bool with_vals, hipStream_t s)
{
    const size_t n = (size_t)nf * cx.tab_sb;
    HIP_TRY(hipMemcpyAsync(e->tab_elem_d, e->tab_elem_h, n * sizeof(int), hipMemcpyHostToDevice, s));
    if (with_vals) HIP_TRY(hipMemcpyAsync(e->tab_val_d, e->tab_val_h, n * sizeof(float), hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(e->ev_tab, s));
    return XFR_OK;
}

xfr_status xfr_ebp_capture(xfr_engine* e, const float* x_dev, int32_t n, int32_t seed_tensor, const float* seed_dev,
                           const int32_t* elem_host, float* p_host, int32_t n_firings, void* stream)
{
    xfr_status st = check_run(e, x_dev, n);
    if (st != XFR_OK) return st;
    if (!seed_dev || !elem_host || !p_host) return fail(XFR_INVALID_ARG, "null argument");
    st = ensure_subtree_scratch(e);
    if (st != XFR_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    BwdPlan* plan = nullptr;
    st = get_plan(e, seed_tensor, &plan);
    if (st != XFR_OK) return st;
    if (n_firings != plan->n_firings) return fail(XFR_INVALID_ARG, "expected %d firings, got %d", plan->n_firings, n_firings);
    SweepCtx cx;
    st = tables_begin(e, cx, n_firings, n);
    if (st != XFR_OK) return st;
    cx.cap_row.assign(n_firings, 0);
    for (int f = 0; f < n_firings; ++f) {
        const Tensor& x = e->tens[plan->firing_tensor[f]];
        for (int b = 0; b < n; ++b) {
            const int el = elem_host[(size_t)f * n + b];
            if (el >= 0 && el < x.per_n()) { e->tab_elem_h[(size_t)f * n + b] = el; cx.cap_row[f] = 1; }
        }
    }
    st = tables_commit(e, cx, n_firings, false, s);
    if (st != XFR_OK) return st;
    HIP_TRY(hipMemsetAsync(e->cap_dev, 0, (size_t)n_firings * n * sizeof(float), s));
    cx.caps = true;
    st = ebp_core(e, cx, x_dev, n, 1, seed_tensor, seed_dev, s);
    if (st != XFR_OK) return st;
    HIP_TRY(hipMemcpyAsync(p_host, e->cap_dev, (size_t)n_firings * n * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return XFR_OK;
}

// the body of xfr_layerwise_ebp; rowmax_key (may be null): the pooled rows go through launch_pool_rowmax, which also leaves each row's max
static xfr_status layerwise_run(xfr_engine* e, const float* x_dev, int32_t n, int32_t n_sweeps, int32_t seed_tensor,
                                const int32_t* firing_host, const int32_t* elem_host, const float* val_host,
                                const float* dense_prior_dev, float* pooled_dev, unsigned* rowmax_key, hipStream_t stream)
{
    xfr_status st = check_run(e, x_dev, n);
    if (st != XFR_OK) return st;
    if (!firing_host || !pooled_dev) return fail(XFR_INVALID_ARG, "null argument");
    const long rows = (long)n_sweeps * n;
    if (n_sweeps < 1 || rows > 2L * e->max_batch)
        return fail(XFR_INVALID_ARG, "%d sweeps x %d images exceed the %d gradient rows of this engine", n_sweeps, n, 2 * e->max_batch);
    if (dense_prior_dev && rows != 1) return fail(XFR_INVALID_ARG, "a dense prior needs one sweep of one image");
    if (!dense_prior_dev && (!elem_host || !val_host)) return fail(XFR_INVALID_ARG, "null prior arrays");
    st = ensure_subtree_scratch(e);
    if (st != XFR_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    BwdPlan* plan = nullptr;
    st = get_plan(e, seed_tensor, &plan);
    if (st != XFR_OK) return st;
    const int nf = plan->n_firings;
    for (long r = 0; r < rows; ++r)
        if (firing_host[r] >= nf || (firing_host[r] < 0 && dense_prior_dev))
            return fail(XFR_INVALID_ARG, "firing %d outside [0, %d)", firing_host[r], nf);
    SweepCtx cx;
    st = tables_begin(e, cx, nf, (int)rows);
    if (st != XFR_OK) return st;
    cx.priors = true;
    cx.prior_row.assign(nf, 0);
    cx.prior_dense = dense_prior_dev;
    if (dense_prior_dev) {
        cx.dense_slot = firing_host[0];
    } else {
        for (long r = 0; r < rows; ++r) {          // row r = sweep j * n + image b; firing < 0: an idle row (stays zero)
            const int f = firing_host[r];
            if (f < 0) continue;
            e->tab_elem_h[(size_t)f * rows + r] = elem_host[r];
            e->tab_val_h[(size_t)f * rows + r] = val_host[r];
            cx.prior_row[f] = 1;
        }
        st = tables_commit(e, cx, nf, true, s);
        if (st != XFR_OK) return st;
    }
    // Sweeps handed over in ascending firing order (per image): sweep j -- identically zero above the earliest of its n priors --
    // only joins the GEMMs and hook chains from the step that holds that prior hook (run_backward: the launches cover a prefix
    // of the gradient rows)
    cx.n = n;
    std::vector<int> first(n_sweeps, nf);
    for (int j = 0; j < n_sweeps; ++j)
        for (int b = 0; b < n; ++b) { const int f = firing_host[(size_t)j * n + b]; if (f >= 0) first[j] = std::min(first[j], f); }
    bool ascending = n_sweeps > 1;
    for (int j = 1; j < n_sweeps; ++j) ascending = ascending && first[j] >= first[j - 1];
    if (ascending && !e->trace_on) cx.active = first;
    // A sweep that is idle for every image (first[j] == nf) never joins the prefix launches, so nothing would write its rows of P[-2]: they are zeroed
    // below, before the sweep (the launches that honour the prefix leave them alone, those that walk every row write the zeros the on-demand zeroing feeds them)
    int live_sweeps = n_sweeps;
    while (live_sweeps > 0 && first[live_sweeps - 1] >= nf) --live_sweeps;
    // one forward for all sweeps (whitebox.py:581 runs ebp(img, 0*P0) again for every layer); zero seeds: all the
    // gradient enters through the priors
    st = forward_all(e, x_dev, n, seed_tensor, true, s);
    if (st != XFR_OK) return st;
    const Tensor& sd = e->tens[seed_tensor];
    // Rows of a gradient tensor that no launch has written must read as zero (a sweep joins at its own firing).  The whole gradient region
    // used to be zero-filled here -- 30 GB at 256 rows, a third of a round; now run_backward zeroes exactly the rows a launch is about to
    // read and nobody has written (XFR_EAGER_ZERO=1: the old fill, for A/B runs; XFR_POISON_G=1, tests: NaN-fill first, so that a row the
    // bookkeeping misses shows up in the maps)
    static const bool eager = getenv("XFR_EAGER_ZERO") != nullptr, poison = getenv("XFR_POISON_G") != nullptr;
    cx.lazy_zero = !cx.active.empty() && !eager;
    if (!cx.active.empty() && (eager || poison))
        HIP_TRY(hipMemsetAsync(e->ws + e->g_begin, eager ? 0 : 0xFF, (e->g_end - e->g_begin) * sizeof(float), s));
    launch_fill(e->G(seed_tensor), (long)sd.per_n() * rows, 0.f, s);
    if (!cx.active.empty() && live_sweeps < n_sweeps) {
        const Tensor& tp = e->tens[1];
        const size_t hw = (size_t)tp.HW();
        (void)hipMemset2DAsync(e->ws + e->tap_off + (size_t)live_sweeps * n * hw, (size_t)rows * hw * sizeof(float), 0,
                               (size_t)(n_sweeps - live_sweeps) * n * hw * sizeof(float), (size_t)tp.C, s);
    }
    st = run_backward(e, cx, *plan, n, n_sweeps, s);
    if (st != XFR_OK) return st;
    const Tensor& t1 = e->tens[1];
    if (rowmax_key)
        launch_pool_rowmax(e->ws + e->tap_off, pooled_dev, rowmax_key, t1.C, (int)rows, t1.HW(), s);
    else
        launch_channel_pool(e->ws + e->tap_off, pooled_dev, t1.C, (int)rows, t1.HW(), s);
    HIP_TRY(hipGetLastError());
    return fence_slot0(e, s);
}

xfr_status xfr_layerwise_ebp(xfr_engine* e, const float* x_dev, int32_t n, int32_t n_sweeps, int32_t seed_tensor,
                             const int32_t* firing_host, const int32_t* elem_host, const float* val_host,
                             const float* dense_prior_dev, float* pooled_dev, void* stream)
{
    return layerwise_run(e, x_dev, n, n_sweeps, seed_tensor, firing_host, elem_host, val_host, dense_prior_dev, pooled_dev, nullptr,
                         (hipStream_t)stream);
}

// xfr_weighted_subtree_ebp's own scratch: row-max keys and gather pairs of a round (2 * max_batch rows), the merge table of n x topk slots and,
// when the caller passes no top_dev, the top-k store (both grown on demand)
static xfr_status ensure_weighted_scratch(xfr_engine* e, int n, int topk, bool need_store)
{
    const size_t rows = 2 * (size_t)e->max_batch;
    if (!e->wst_key_d) {
        DevBuf<unsigned> key_d;
        PinnedBuf<unsigned> key_h;
        DevBuf<int> pairs_d, cnt_d;
        PinnedBuf<int> pairs_h, cnt_h;
        XFR_TRY(key_d.alloc(rows));
        XFR_TRY(key_h.alloc(rows));
        XFR_TRY(pairs_d.alloc(2 * rows));
        XFR_TRY(pairs_h.alloc(2 * rows));
        XFR_TRY(cnt_d.alloc((size_t)e->max_batch));
        XFR_TRY(cnt_h.alloc((size_t)e->max_batch));
        e->wst_key_d = std::move(key_d); e->wst_key_h = std::move(key_h); e->wst_pairs_d = std::move(pairs_d);
        e->wst_pairs_h = std::move(pairs_h); e->wst_cnt_d = std::move(cnt_d); e->wst_cnt_h = std::move(cnt_h);
    }
    const size_t slots = (size_t)n * topk;
    if (slots > e->wst_tab_d.cap) {
        e->wst_tab_d.reset();
        e->wst_tab_h.reset();
        DevBuf<SubtreeSlot> tab_d;
        PinnedBuf<SubtreeSlot> tab_h;
        XFR_TRY(tab_d.alloc(slots));
        XFR_TRY(tab_h.alloc(slots));
        e->wst_tab_d = std::move(tab_d); e->wst_tab_h = std::move(tab_h);
    }
    const size_t floats = slots * (size_t)e->tens[1].HW();
    if (need_store && floats > e->wst_store.cap) XFR_TRY(e->wst_store.alloc(floats));
    return XFR_OK;
}

xfr_status xfr_weighted_subtree_ebp(xfr_engine* e, const float* x_dev, int32_t n, int32_t seed_tensor, const float* seed_dev,
                                    const xfr_subtree_args* args, float* smap_dev, float* top_dev, float* w_valid_host,
                                    int32_t* k_valid_host, int32_t* n_valid_host, void* stream)
{
    static const char* const mode_names[4] = {"affineonly", "affineonly_with_prior", "norelu", "all"};
    xfr_status st = check_run(e, x_dev, n);
    if (st != XFR_OK) return st;
    if (!seed_dev || !args || !smap_dev || !w_valid_host || !k_valid_host || !n_valid_host) return fail(XFR_INVALID_ARG, "null argument");
    const int topk = args->topk;
    if (topk < 1) return fail(XFR_INVALID_ARG, "xfr_weighted_subtree_ebp: topk %d, must be >= 1", topk);
    if (args->output < XFR_SUBTREE_MWP || args->output > XFR_SUBTREE_UINT8_SALIENCY)
        return fail(XFR_INVALID_ARG, "xfr_weighted_subtree_ebp: output %d is not an xfr_subtree_output", args->output);
    if (args->output == XFR_SUBTREE_UINT8_SALIENCY && (long)e->tens[1].H * e->tens[1].W > U8_TAIL_MAX_HW)
        return fail(XFR_INVALID_ARG, "xfr_weighted_subtree_ebp: maps of %d x %d exceed the %d pixels of the uint8 tail", e->tens[1].H, e->tens[1].W,
                    U8_TAIL_MAX_HW);
    if (args->sweep_batch < 0) return fail(XFR_INVALID_ARG, "xfr_weighted_subtree_ebp: sweep_batch %d < 0", args->sweep_batch);
    if (seed_tensor < 2 || seed_tensor >= (int)e->tens.size()) return fail(XFR_INVALID_ARG, "bad seed tensor %d", seed_tensor);
    // whitebox.py's first round: min(2 * max_batch / N, max(8, 2 * topk)) candidates per probe
    const long J = args->sweep_batch > 0 ? (long)args->sweep_batch
                                         : std::max(1L, std::min((2L * e->max_batch) / n, (long)std::max(8, 2 * topk)));
    if (J * n > 2L * e->max_batch)
        return fail(XFR_INVALID_ARG, "xfr_weighted_subtree_ebp: %ld sweeps x %d images exceed the %d gradient rows of this engine", J, n,
                    2 * e->max_batch);
    st = ensure_subtree_scratch(e);
    if (st != XFR_OK) return st;
    st = ensure_weighted_scratch(e, n, topk, top_dev == nullptr);
    if (st != XFR_OK) return st;
    BwdPlan* plan = nullptr;
    st = get_plan(e, seed_tensor, &plan);
    if (st != XFR_OK) return st;
    const int nf = plan->n_firings;
    const Tensor& t1 = e->tens[1];
    const int HW = t1.HW();
    const size_t D = (size_t)e->tens[seed_tensor].per_n();
    hipStream_t s = (hipStream_t)stream;
    float* store = top_dev ? top_dev : e->wst_store;

    // 1. one forward for every phase; the caller's hold (an enclosing group) survives the call, ours ends with it
    HoldGuard hold(e);

    // 2-3. layer weights, chosen elements and prior values
    std::vector<float> w((size_t)nf * n), vals((size_t)nf * n);
    std::vector<int> idx((size_t)nf * n);
    st = xfr_subtree_weights(e, x_dev, n, seed_tensor, seed_dev, args->gate_ge0, w.data(), idx.data(), nf * n, stream);
    if (st != XFR_OK) return st;
    st = xfr_ebp_capture(e, x_dev, n, seed_tensor, seed_dev + 2 * (size_t)n * D, idx.data(), vals.data(), nf, stream);
    if (st != XFR_OK) return st;

    // 4. visiting orders, ascending by weight
    std::vector<std::vector<int>> order(n, std::vector<int>(nf));
    {
        std::vector<float> col(nf);
        std::vector<char> seen(nf);
        for (int b = 0; b < n; ++b) {
            for (int k = 0; k < nf; ++k) col[k] = w[(size_t)k * n + b];
            std::vector<int>& o = order[b];
            if (args->order_fn) {
                const int32_t r = args->order_fn(col.data(), nf, b, o.data(), args->order_user);
                if (r != 0) return fail(XFR_INVALID_ARG, "xfr_weighted_subtree_ebp: order_fn returned %d for probe %d", r, b);
                std::fill(seen.begin(), seen.end(), 0);
                for (int k = 0; k < nf; ++k) {
                    if (o[k] < 0 || o[k] >= nf || seen[o[k]])
                        return fail(XFR_INVALID_ARG, "xfr_weighted_subtree_ebp: order_fn gave no permutation of the %d firings (probe %d)", nf, b);
                    seen[o[k]] = 1;
                }
            } else {
                // np.argsort(w.astype(np.float64), kind='stable'); NaN sorts last like NumPy's
                for (int k = 0; k < nf; ++k) o[k] = k;
                std::stable_sort(o.begin(), o.end(), [&](int a, int c) {
                    const double x = col[a], y = col[c];
                    return x < y || (x == x && y != y);
                });
            }
        }
    }

    // 5-6. rounds of layerwise sweeps from the heaviest firing down (whitebox.py:700-716 as _weighted_subtree evaluates it)
    std::vector<int> pos(n, nf);
    std::vector<std::vector<int>> valid(n);          // per probe: valid firings, heaviest first; slot i of the store holds valid[b][i]
    std::vector<std::vector<float>> vmax(n);         // ... and the max of each of those maps
    std::vector<std::vector<int>> ks(n), row(n);
    std::vector<int> F, E;
    std::vector<float> V;
    std::vector<long> lim(n);
    float* pooled = e->ws + e->pooled_off;          // 2 * max_batch maps
    if (top_dev) HIP_TRY(hipMemsetAsync(top_dev, 0, (size_t)n * topk * HW * sizeof(float), s));
    int rounds = 0;
    for (;;) {
        bool open = false;
        for (int b = 0; b < n; ++b) open = open || (pos[b] > 0 && (int)valid[b].size() < topk);
        if (!open) break;
        long Jr = 1;
        for (int b = 0; b < n; ++b) {
            lim[b] = rounds == 0 ? J : std::min(J, 2L * (topk - (long)valid[b].size()) + 2);
            if ((int)valid[b].size() < topk) Jr = std::max(Jr, lim[b]);
        }
        ++rounds;
        F.assign((size_t)Jr * n, -1);
        E.assign((size_t)Jr * n, 0);
        V.assign((size_t)Jr * n, 0.f);
        bool work = false;
        for (int b = 0; b < n; ++b) {
            ks[b].clear();
            if ((int)valid[b].size() < topk) {
                while (pos[b] > 0 && (long)ks[b].size() < lim[b]) {
                    const int k = order[b][--pos[b]];
                    if (vals[(size_t)k * n + b] != 0.f && k != 1) ks[b].push_back(k);     // an all-zero prior gives an all-zero map (:706); k == 1 (:707)
                }
            }
            std::vector<int> asc = ks[b];
            std::sort(asc.begin(), asc.end());                     // ascending firing: a sweep joins at its own firing
            row[b].assign(ks[b].size(), 0);
            for (size_t j = 0; j < asc.size(); ++j) {
                const int k = asc[j];
                F[j * n + b] = k;
                E[j * n + b] = idx[(size_t)k * n + b];
                V[j * n + b] = vals[(size_t)k * n + b];
                for (size_t q = 0; q < ks[b].size(); ++q) if (ks[b][q] == k) row[b][q] = (int)(j * n + b);
            }
            work = work || !ks[b].empty();
        }
        if (!work) continue;
        st = layerwise_run(e, x_dev, n, (int)Jr, seed_tensor, F.data(), E.data(), V.data(), nullptr, pooled, e->wst_key_d, s);
        if (st != XFR_OK) return st;
        HIP_TRY(hipMemcpyAsync(e->wst_key_h, e->wst_key_d, (size_t)Jr * n * sizeof(unsigned), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));                 // also: the previous round's pairs have left wst_pairs_h
        int np = 0;
        for (int b = 0; b < n; ++b)
            for (size_t q = 0; q < ks[b].size(); ++q) {
                const float m = rowmax_from_key(e->wst_key_h[row[b][q]]);
                if (m > 0.f && (int)valid[b].size() < topk) {                          // np.max(P) > 0 (:706)
                    e->wst_pairs_h[2 * np] = row[b][q];
                    e->wst_pairs_h[2 * np + 1] = b * topk + (int)valid[b].size();
                    ++np;
                    valid[b].push_back(ks[b][q]);
                    vmax[b].push_back(m);
                }
            }
        if (np > 0) {
            HIP_TRY(hipMemcpyAsync(e->wst_pairs_d, e->wst_pairs_h, 2 * (size_t)np * sizeof(int), hipMemcpyHostToDevice, s));
            launch_gather_rows(pooled, store, e->wst_pairs_d, np, HW, s);
        }
    }
    for (int b = 0; b < n; ++b)
        if (valid[b].empty())
            return fail(XFR_STATE_ERROR, "Failed to calculate valid subtrees. The ebp subtree mode (%s) may not support by this type of network. "
                        "You may want to try the \"affineonly_with_prior\" ebp subtree mode.", mode_names[e->mode & 3]);

    // 7. the merge table in the reference's order (ascending weight): scale-normalised weights (_scale_normalized, fp32) and 1 / (max + 1e-12)
    for (int b = 0; b < n; ++b) {
        const int c = (int)valid[b].size();
        e->wst_cnt_h[b] = c;
        n_valid_host[b] = c;
        float mn = INFINITY, mx = -INFINITY;
        for (int t = 0; t < topk; ++t) {
            k_valid_host[(size_t)b * topk + t] = -1;
            w_valid_host[(size_t)b * topk + t] = 0.f;
        }
        for (int t = 0; t < c; ++t) {
            const int k = valid[b][c - 1 - t];
            const float wk = w[(size_t)k * n + b];
            k_valid_host[(size_t)b * topk + t] = k;
            w_valid_host[(size_t)b * topk + t] = wk;
            mn = std::min(mn, wk);
            mx = std::max(mx, wk);
        }
        const float den = e->eps + (mx - mn);
        bool all_zero = true;
        for (int t = 0; t < c; ++t) {
            const float sn = (w_valid_host[(size_t)b * topk + t] - mn) / den;
            all_zero = all_zero && sn == 0.f;
            e->wst_tab_h[(size_t)b * topk + t] = SubtreeSlot{c - 1 - t, sn, 1.0f / (vmax[b][c - 1 - t] + 1e-12f), 0};
        }
        if (all_zero)
            for (int t = 0; t < c; ++t) e->wst_tab_h[(size_t)b * topk + t].wn = 1.0f;       // np.sum(sn) == 0 -> ones (:718)
    }
    HIP_TRY(hipMemcpyAsync(e->wst_tab_d, e->wst_tab_h, (size_t)n * topk * sizeof(SubtreeSlot), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(e->wst_cnt_d, e->wst_cnt_h, (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
    launch_subtree_merge(store, e->wst_tab_d, e->wst_cnt_d, smap_dev, n, topk, HW, args->do_max_subtree ? 1 : 0,
                         (args->output == XFR_SUBTREE_UINT8 || args->output == XFR_SUBTREE_UINT8_SALIENCY) ? 1 : 0, e->eps, s);
    if (top_dev) launch_reverse_slots(top_dev, e->wst_cnt_d, n, topk, HW, s);
    // 8. _mwp_to_saliency (ebp_version 6) of the merged map and the top-k maps, in place
    if (args->output == XFR_SUBTREE_SALIENCY) {
        float* tmp = e->ws + e->blur_b_off;                // 2 * max_batch maps
        launch_saliency_blur(smap_dev, tmp, smap_dev, n, t1.H, t1.W, e->eps, s);
        if (top_dev) {
            const long maps = (long)n * topk, cap = 2L * e->max_batch;
            for (long r0 = 0; r0 < maps; r0 += cap)
                launch_saliency_blur(top_dev + r0 * HW, tmp, top_dev + r0 * HW, (int)std::min(cap, maps - r0), t1.H, t1.W, e->eps, s);
        }
    }
    // ... and of the other versions (whitebox.py:451-454), in place: the merged map holds uint8 levels and takes the uint8 form of the first
    // stretch, the top-k maps are float32 maps (an empty slot is constant, hence stays zero); both come back as levels held in floats
    if (args->output == XFR_SUBTREE_UINT8_SALIENCY) {
        launch_u8_tail(smap_dev, nullptr, true, nullptr, smap_dev, n, t1.H, t1.W, e->eps, s);
        if (top_dev) launch_u8_tail(top_dev, nullptr, false, nullptr, top_dev, n * topk, t1.H, t1.W, e->eps, s);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    return XFR_OK;
}

xfr_status xfr_ebp_store_firing(xfr_engine* e, const float* x_dev, int32_t n, int32_t seed_tensor, const float* seed_dev,
                                int32_t firing, float* out_dev, int32_t* c, int32_t* h, int32_t* w, void* stream)
{
    xfr_status st = check_run(e, x_dev, n);
    if (st != XFR_OK) return st;
    if (!seed_dev) return fail(XFR_INVALID_ARG, "null seed");
    st = ensure_subtree_scratch(e);
    if (st != XFR_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    BwdPlan* plan = nullptr;
    st = get_plan(e, seed_tensor, &plan);
    if (st != XFR_OK) return st;
    if (firing < 0 || firing > plan->n_firings) return fail(XFR_INVALID_ARG, "firing %d outside [0, %d]", firing, plan->n_firings);
    if (firing == plan->n_firings) {
        // the image hook, Whitebox.P[-1]: one standard sweep leaves the gradient of the first convolution's output (after its hooks) in G(1);
        // its backward-data pass with relu(W) and the hook p = relu(image) * relu(z) run as one gather kernel (nothing on the path reads this)
        if (c) *c = e->in_c;
        if (h) *h = e->in_h;
        if (w) *w = e->in_w;
        if (!out_dev) return XFR_OK;
        {
            // un-pipelined on purpose: the gather below reads the image from forward slot 0 on the caller's stream; a pipelined call would have
            // put it into slot seq % n_slots on an internal stream (and ebp_core resets cur_slot before it returns)
            Scoped<bool> unpipe(e->pipeline_all, false);
            st = ebp_core(e, SweepCtx(), x_dev, n, 1, seed_tensor, seed_dev, s);
        }
        if (st != XFR_OK) return st;
        const OpRec& o = e->ops[0];
        const xfr_op_desc& d = o.d;
        const Tensor& t1 = e->tens[d.out];
        launch_image_mwp(e->G(d.out), e->arena + o.w_pos, e->T(0), out_dev, e->in_c, n, e->in_h, e->in_w, d.cout, t1.H, t1.W, d.kh, d.kw, d.stride,
                         d.pad, o.ldw, o.tap4_fwd ? 2 : (o.tap_fwd ? 1 : 0), o.pair, s);
        HIP_TRY(hipGetLastError());
        return fence_slot0(e, s);           // the gather still reads slot 0: a later pipelined forward into it waits for THIS point
    }
    const Tensor& x = e->tens[plan->firing_tensor[firing]];
    if (c) *c = x.C;
    if (h) *h = x.H;
    if (w) *w = x.W;
    if (!out_dev) return XFR_OK;          // shape query
    const bool is_tap = (firing == plan->n_firings - 1);
    SweepCtx cx;
    if (!is_tap) { cx.store_slot = firing; cx.store_dst = e->store_dev; }
    st = ebp_core(e, cx, x_dev, n, 1, seed_tensor, seed_dev, s);
    if (st != XFR_OK) return st;
    launch_cnhw_to_nchw(is_tap ? e->ws + e->tap_off : e->store_dev, out_dev, n, x.C, x.HW(), s);
    HIP_TRY(hipGetLastError());
    return XFR_OK;
}

}  // extern "C"
