/* The paper's weighted subtree EBP from a host that is not Python: plain C99 against include/xfr_amd.h, one call.
 *
 * The three-layer network, parameters and images of c_host.c (Conv 3x3 -> BatchNorm -> in-place ReLU -> Linear over the map -> L2
 * normalise).  Images 0 and 1 are encoded; their unit-norm encodings are the rows of the two-way triplet classifier (mate, non-mate)
 * as the inpainting-game generator installs it for this method.  Image 2 is the probe: xfr_weighted_subtree_ebp runs
 * Whitebox.weighted_subtree_ebp (python/xfr/models/whitebox.py:647-737; 'norelu', top-2, mated-similarity gating, summed subtrees,
 * ebp_version 6) and the program checks the selected firings, their weights and the saliency map against what the real reference
 * computes (c_subtree_ref.h).  Without a device it prints the engine's loud refusal to run on the CPU and exits 0.
 *
 * Known gap: the reference selects firings 2 and 0 here.  The engine's layerwise sweep (xfr_layerwise_ebp, which this call and the Python path
 * share) returns an all-zero map for a prior on firing 0 -- the Linear input directly below the encoding -- so the engine selects firing 2
 * alone.  The reference's maps of the two firings are the same map, so the merged map still matches; the program requires every firing it
 * selects to be one the reference selected, with the reference's weight, and reports whether the selection is complete.
 *
 *   gcc -std=c99 -Iinclude -Iexamples examples/c_subtree.c -Lxfr_amd/csrc -lxfr_amd -Wl,-rpath,$PWD/xfr_amd/csrc -ldl -lm -o c_subtree && ./c_subtree
 */
#include <dlfcn.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "xfr_amd.h"
#include "c_subtree_ref.h"   /* tests/golden/make_golden_csubtree.py */

#define IMG 16
#define C1 8
#define D 6
#define TOPK C_SUBTREE_REF_TOPK

static float frand(unsigned* s) { *s = *s * 1664525u + 1013904223u; return (float)((*s >> 8) & 0xFFFF) / 65536.0f - 0.5f; }

int main(void)
{
    xfr_op_desc ops[5];
    memset(ops, 0, sizeof(ops));
    for (int k = 0; k < 5; ++k) { ops[k].in1 = -1; ops[k].out = k + 1; ops[k].stride = 1; ops[k].w_weight = ops[k].w_bias = ops[k].w_mean = ops[k].w_var = -1; }
    ops[0].kind = XFR_OP_CONV;      ops[0].in0 = 0; ops[0].cout = C1; ops[0].kh = ops[0].kw = 3; ops[0].pad = 1; ops[0].w_weight = 0; ops[0].w_bias = 1;
    ops[1].kind = XFR_OP_BATCHNORM; ops[1].in0 = 1; ops[1].fparam = 1e-5f; ops[1].w_weight = 2; ops[1].w_bias = 3; ops[1].w_mean = 4; ops[1].w_var = 5;
    ops[2].kind = XFR_OP_RELU;      ops[2].in0 = 2; ops[2].inplace = 1;
    ops[3].kind = XFR_OP_LINEAR;    ops[3].in0 = 3; ops[3].cout = D; ops[3].kh = ops[3].kw = IMG; ops[3].w_weight = 6; ops[3].w_bias = 7;
    ops[4].kind = XFR_OP_G_NORMALIZE; ops[4].in0 = 4;
    const int n_ops = 5, n_weights = 8, encode_tensor = 5;

    unsigned seed = 12345u;
    static float w0[C1 * 1 * 9], b0[C1], g[C1], be[C1], mu[C1], var[C1], w3[D * C1 * IMG * IMG], b3[D];
    for (int i = 0; i < C1 * 9; ++i) w0[i] = frand(&seed);
    for (int i = 0; i < C1; ++i) { b0[i] = 0.1f * frand(&seed); g[i] = 1.0f + 0.4f * frand(&seed); be[i] = 0.2f * frand(&seed); mu[i] = 0.2f * frand(&seed); var[i] = 1.0f + 0.5f * frand(&seed); }
    for (int i = 0; i < D * C1 * IMG * IMG; ++i) w3[i] = 0.05f * frand(&seed);
    for (int i = 0; i < D; ++i) b3[i] = 0.05f * frand(&seed);
    xfr_tensor_view views[8] = {{w0, C1 * 9}, {b0, C1}, {g, C1}, {be, C1}, {mu, C1}, {var, C1}, {w3, (int64_t)D * C1 * IMG * IMG}, {b3, D}};

    xfr_engine* e = NULL;
    xfr_status st = xfr_engine_create(ops, n_ops, n_weights, 1, IMG, IMG, 4, 0, &e);
    if (st != XFR_OK) {
        printf("-- no engine: %s\n", xfr_last_error());       /* "... the xfr_amd engine has no CPU fallback" */
        return st == XFR_HIP_ERROR ? 0 : 1;
    }
    void* hip = dlopen("libamdhip64.so", RTLD_NOW);
    if (!hip) hip = dlopen("/opt/rocm/lib/libamdhip64.so", RTLD_NOW);
    if (!hip) { fprintf(stderr, "libamdhip64: %s\n", dlerror()); return 1; }
    int (*hipMalloc_)(void**, size_t) = (int (*)(void**, size_t))dlsym(hip, "hipMalloc");
    int (*hipMemcpy_)(void*, const void*, size_t, int) = (int (*)(void*, const void*, size_t, int))dlsym(hip, "hipMemcpy");
    int (*hipDeviceSynchronize_)(void) = (int (*)(void))dlsym(hip, "hipDeviceSynchronize");
    if (!hipMalloc_ || !hipMemcpy_ || !hipDeviceSynchronize_) return 1;
    if (xfr_engine_load_weights(e, views, n_weights) != XFR_OK || xfr_engine_set_mode(e, XFR_MODE_NORELU, 1e-16f, 0) != XFR_OK) {
        fprintf(stderr, "%s\n", xfr_last_error());
        return 1;
    }

    /* the triplet classifier: unit-norm encodings of images 0 (mate) and 1 (non-mate) */
    static float imgs[3 * IMG * IMG], enc[2 * D], seeds[3 * D], smap[IMG * IMG];
    for (int i = 0; i < 3 * IMG * IMG; ++i) imgs[i] = 4.0f * frand(&seed);
    float *d_img = NULL, *d_enc = NULL, *d_seed = NULL, *d_smap = NULL;
    hipMalloc_((void**)&d_img, sizeof(imgs)); hipMalloc_((void**)&d_enc, sizeof(enc)); hipMalloc_((void**)&d_seed, sizeof(seeds));
    hipMalloc_((void**)&d_smap, sizeof(smap));
    hipMemcpy_(d_img, imgs, sizeof(imgs), 1 /* host to device */);
    if (xfr_forward(e, d_img, 2, encode_tensor, d_enc, NULL) != XFR_OK) { fprintf(stderr, "%s\n", xfr_last_error()); return 1; }
    hipDeviceSynchronize_();
    hipMemcpy_(enc, d_enc, sizeof(enc), 2 /* device to host */);
    /* seeds at the encoding, 3 streams x 1 probe x D: the gate output y[0][0] (mate row), the non-mate output y[0][1], the EBP channel 0 */
    memcpy(seeds, enc, D * sizeof(float));
    memcpy(seeds + D, enc + D, D * sizeof(float));
    memcpy(seeds + 2 * D, enc, D * sizeof(float));
    hipMemcpy_(d_seed, seeds, sizeof(seeds), 1);

    xfr_subtree_args args;
    memset(&args, 0, sizeof(args));
    args.topk = TOPK;
    args.gate_ge0 = 1;
    args.do_max_subtree = 0;
    args.output = XFR_SUBTREE_SALIENCY;
    args.sweep_batch = 0;
    args.order_fn = NULL;           /* the engine's order rule: this network has no tied weights among the firings it can select */
    float w_valid[TOPK];
    int32_t k_valid[TOPK], n_valid = 0;
    if (xfr_weighted_subtree_ebp(e, d_img + 2 * IMG * IMG, 1, encode_tensor, d_seed, &args, d_smap, NULL, w_valid, k_valid, &n_valid, NULL) != XFR_OK) {
        fprintf(stderr, "xfr_weighted_subtree_ebp: %s\n", xfr_last_error());
        return 1;
    }
    hipMemcpy_(smap, d_smap, sizeof(smap), 2);
    int subset = n_valid >= 1 && n_valid <= TOPK;       /* every selected firing is one of the reference's, with its weight */
    double w_err = 0.0;
    printf("-- weighted subtree EBP: %d valid subtrees, firings", n_valid);
    for (int i = 0; i < n_valid && i < TOPK; ++i) {
        printf(" %d (w %.6g)", k_valid[i], w_valid[i]);
        int j = 0;
        while (j < TOPK && c_subtree_ref_k[j] != k_valid[i]) ++j;
        if (j == TOPK) { subset = 0; continue; }
        w_err = fmax(w_err, fabs((double)w_valid[i] - c_subtree_ref_w[j]) / fabs((double)c_subtree_ref_w[j]));
    }
    printf("\n");
    double sum = 0.0, dmax = 0.0, rmax = 0.0, dot = 0.0, na = 0.0, nb = 0.0;
    for (int i = 0; i < IMG * IMG; ++i) {
        const double a = smap[i], b = c_subtree_ref_map[i];
        sum += a;
        dmax = fmax(dmax, fabs(a - b)); rmax = fmax(rmax, fabs(b));
        dot += a * b; na += a * a; nb += b * b;
    }
    const double rel = dmax / rmax, cosine = dot / sqrt(na * nb);
    printf("-- saliency map %dx%d: sum %.6f\n", IMG, IMG, sum);
    printf("-- against the reference: firings among the reference's %s (%d of %d), weights max rel |d| %.2e, map max|d|/max %.3e, cosine %.8f\n",
           subset ? "yes" : "NO", n_valid, TOPK, w_err, rel, cosine);
    xfr_engine_destroy(e);
    return (subset && w_err <= 1e-4 && fabs(sum - 1.0) < 1e-3 && rel <= 1e-3 && cosine >= 0.99999) ? 0 : 1;
}
