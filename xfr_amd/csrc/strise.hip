// strise.hip -- the device side of STRise blackbox saliency (python/xfr/models/blackbox.py:299-442): sparse masks, masked probes, triplet scores and the
// weighted merge.  A mask is never stored on the sweep and merge paths: it is a function of its drawn cells and its shift, evaluated in float64 where
// it is needed.  The mask law (blackbox.py:333, skimage.transform.resize(order=1, mode='reflect', anti_aliasing=False) of skimage >= 0.19, i.e.
// scipy.ndimage.zoom(order=1, mode='mirror', grid_mode=True)), for output row r of a mask with shift (x, y):
//     c  = (r + x + 0.5) * (gh / (H + s)) - 0.5,  i0 = floor(c),  f = c - i0      (columns alike with y, gw, W)
//     rows i0 and i0 + 1 through the mirror map  i -> |i| mod 2 (gh - 1), folded at gh - 1
//     mask = bilinear blend of the four grid values (1 everywhere, 0 at the drawn cells)
// The host side (argument checks, batching, streams) is strise_abi.hip.
#include "common.h"
#include <math.h>

namespace {

constexpr int NT = 256;

__device__ inline int mirror_index(int i, int g)
{
    if (g == 1) return 0;
    const int p = 2 * (g - 1);
    i = (i < 0 ? -i : i) % p;
    return i > g - 1 ? p - i : i;
}

// A mask law is stated once, as a type with  taps(o, g, ratio) -> the two taps i0, i1 and their weights w0, w1  for output coordinate o (shift
// included) of an axis with g cells,  value(the four grid values, the row's weights, the column's weights)  and what a probe pixel becomes under
// it: pixel(mask, probe, fill) and input(pixel, mean), the network's fp32 input.  ratio = g / (size + scale), divided once on the host -- the order
// in which scipy's zoom evaluates the coordinate.

// The law above in closed form, as the float64 sweep and the merge evaluate it: w1 is the coordinate's fraction, and value() takes one minus it
// where it multiplies instead of reading w0 (the __d*_rn of the HIP headers contract with their surroundings: these expressions stay as they are)
struct ClosedLaw {
    static __device__ inline void taps(int o, int g, double ratio, int& i0, int& i1, double& w0, double& w1)
    {
        const double c = __dsub_rn(__dmul_rn((double)o + 0.5, ratio), 0.5);
        const double fl = floor(c);
        w1 = c - fl;
        w0 = 1.0 - w1;
        i0 = mirror_index((int)fl, g);
        i1 = mirror_index((int)fl + 1, g);
    }

    static __device__ inline double value(double v00, double v01, double v10, double v11, double, double fy, double, double fx)
    {
        const double top = __dadd_rn(__dmul_rn(1.0 - fx, v00), __dmul_rn(fx, v01));
        const double bot = __dadd_rn(__dmul_rn(1.0 - fx, v10), __dmul_rn(fx, v11));
        return __dadd_rn(__dmul_rn(1.0 - fy, top), __dmul_rn(fy, bot));
    }

    // blackbox.py:343 and resnet.py:32,37: mask * u8 + (1 - mask) * fill, then (float)(v - mean[c]), in float64
    static __device__ inline double pixel(double m, double p, double f) { return __dadd_rn(__dmul_rn(m, p), __dmul_rn(__dsub_rn(1.0, m), f)); }
    static __device__ inline float input(double v, double mean) { return (float)__dsub_rn(v, mean); }
};

// The mask law of the generator's black box (eval/generate_inpaintinggame_bb_saliency_maps_multigpu.py:73-101): every masked probe goes through
// Whitebox.convert_from_numpy (whitebox.py:787-806), which TRUNCATES (v / 255) * 255 to uint8 -- a mask that is 1 - 2^-53 where the closed form gives
// 1 costs a level.  So this law evaluates scipy's zoom to the bit: one rounded float64 operation per step (common.h), none contracted.  A row of
// the image list whose shift is negative has no mask (image zero: the unmasked probe, and the padding): q = probe, since
// uint8((k / 255) * 255) == k for every level and an all-ones mask under this law is not the probe.
struct ExactLaw {
    // scipy.ndimage.zoom(order=1, mode='mirror', grid_mode=True) along one axis of g cells, output coordinate o (shift included): only a negative
    // coordinate is reflected, the second spline weight is one minus the first (not the fraction), the upper tap folds at g - 1
    static __device__ inline void taps(int o, int g, double ratio, int& i0, int& i1, double& w0, double& w1)
    {
        const double cc = sub_rn(mul_rn((double)o + 0.5, ratio), 0.5);
        const double c = cc < 0.0 ? -cc : cc;
        const double st = floor(c);
        w0 = sub_rn(1.0, sub_rn(c, st));
        w1 = sub_rn(1.0, w0);
        i0 = min((int)st, g - 1);
        i1 = i0 + 1;
        if (i1 > g - 1) i1 = 2 * (g - 1) - i1;
        if (g == 1) { i0 = i1 = 0; w0 = 1.0; w1 = 0.0; }
    }

    // scipy's accumulation: from 0.0, rows outermost, each product as (G * wy) * wx
    static __device__ inline double value(double g00, double g01, double g10, double g11, double wy0, double wy1, double wx0, double wx1)
    {
        double t = add_rn(0.0, mul_rn(mul_rn(g00, wy0), wx0));
        t = add_rn(t, mul_rn(mul_rn(g01, wy0), wx1));
        t = add_rn(t, mul_rn(mul_rn(g10, wy1), wx0));
        return add_rn(t, mul_rn(mul_rn(g11, wy1), wx1));
    }

    // blackbox.py:343 then whitebox.py:794-795,803: np.uint8((v / 255) * 255) of v = mask * probe + (1 - mask) * fill, an IEEE division and
    // product, truncated (v lies in [0, 255]); then (float)((double)q - mean[c])
    static __device__ inline int pixel(double m, double p, double f)
    {
        const double v = add_rn(mul_rn(m, p), mul_rn(sub_rn(1.0, m), f));
        return (int)mul_rn(div_rn(v, 255.0), 255.0);
    }
    static __device__ inline float input(int q, double mean) { return (float)sub_rn((double)q, mean); }
};

// the grid of one mask in LDS: 1 everywhere, 0 at its cells (cell < 0: no cell -- the all-ones mask of the unmasked probe and of the padding)
__device__ inline void build_grid(uint8_t* grid, const int* __restrict__ cells, int n_elem, int cells_total)
{
    for (int i = threadIdx.x; i < cells_total; i += blockDim.x) grid[i] = 1;
    __syncthreads();
    for (int i = threadIdx.x; i < n_elem; i += blockDim.x) {
        const int c = cells[i];
        if (c >= 0 && c < cells_total) grid[c] = 0;
    }
    __syncthreads();
}

// K_strise_masked: the fp32 network input of a batch of masked probes under the closed law, NCHW.  One thread: four pixels of a row, the mask once
// per pixel, three channels; float4 stores along W.  Eight waves per SIMD (64 VGPRs, 63 used): the kernel runs beside the forward of the batch
// before and must not take its occupancy.
__global__ __launch_bounds__(NT, 8) void strise_masked_kernel(const uint8_t* __restrict__ probe, const double* __restrict__ fill, const int* __restrict__ cells,
                                                           const int* __restrict__ shifts, float* __restrict__ out, StriseGeom g, double m0, double m1, double m2)
{
    __shared__ uint8_t grid[STRISE_MAX_CELLS];
    const int k = blockIdx.y;
    build_grid(grid, cells + (size_t)k * g.n_elem, g.n_elem, g.gh * g.gw);
    const int W4 = (g.W + 3) >> 2;
    const int q = blockIdx.x * NT + threadIdx.x;
    if (q >= g.H * W4) return;
    const int row = q / W4, x0 = (q - row * W4) * 4;
    const int sx = shifts[2 * k], sy = shifts[2 * k + 1];
    double m[4];
    int r0, r1;
    double wy0, wy1;
    ClosedLaw::taps(row + sx, g.gh, g.ry, r0, r1, wy0, wy1);
    const uint8_t* g0 = grid + r0 * g.gw;
    const uint8_t* g1 = grid + r1 * g.gw;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int c0, c1;
        double wx0, wx1;
        ClosedLaw::taps(min(x0 + j, g.W - 1) + sy, g.gw, g.rx, c0, c1, wx0, wx1);
        m[j] = ClosedLaw::value((double)g0[c0], (double)g0[c1], (double)g1[c0], (double)g1[c1], wy0, wy1, wx0, wx1);
    }
    const double mean[3] = {m0, m1, m2};
    const size_t plane = (size_t)g.H * g.W;
    const size_t px = ((size_t)row * g.W + x0) * 3;
    float* o = out + (size_t)k * 3 * plane + (size_t)row * g.W + x0;
    const bool vec = (g.W & 3) == 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const size_t at = px + 3 * (vec ? j : min(j, g.W - 1 - x0)) + c;
            v[j] = ClosedLaw::input(ClosedLaw::pixel(m[j], (double)probe[at], fill[at]), mean[c]);
        }
        if (vec) {
            *reinterpret_cast<float4*>(o + c * plane) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            for (int j = 0; j < 4 && x0 + j < g.W; ++j) o[c * plane + j] = v[j];
        }
    }
}

// K_strise_quant: strise_masked_kernel for the quantised chain, under the exact law.  U8OUT: the parity hook, q itself as uint8 H x W x 3; else
// the network input, NCHW, float4 stores.  The two stay two kernels: as one template over (law, output) the closed-law instantiation came out in
// another register assignment, and strise_masked_kernel sits one register under its limit.
template <bool U8OUT>
__global__ __launch_bounds__(NT, 8) void strise_quant_kernel(const uint8_t* __restrict__ probe, const double* __restrict__ fill, const int* __restrict__ cells,
                                                          const int* __restrict__ shifts, void* __restrict__ out_any, StriseGeom g, double m0, double m1, double m2)
{
    __shared__ uint8_t grid[STRISE_MAX_CELLS];
    const int k = blockIdx.y;
    build_grid(grid, cells + (size_t)k * g.n_elem, g.n_elem, g.gh * g.gw);
    const int W4 = (g.W + 3) >> 2;
    const int q = blockIdx.x * NT + threadIdx.x;
    if (q >= g.H * W4) return;
    const int row = q / W4, x0 = (q - row * W4) * 4;
    const int sx = shifts[2 * k], sy = shifts[2 * k + 1];
    const bool masked = sx >= 0;
    double m[4] = {1.0, 1.0, 1.0, 1.0};
    if (masked) {
        int r0, r1;
        double wy0, wy1;
        ExactLaw::taps(row + sx, g.gh, g.ry, r0, r1, wy0, wy1);
        const uint8_t* g0 = grid + r0 * g.gw;
        const uint8_t* g1 = grid + r1 * g.gw;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int c0, c1;
            double wx0, wx1;
            ExactLaw::taps(min(x0 + j, g.W - 1) + sy, g.gw, g.rx, c0, c1, wx0, wx1);
            m[j] = ExactLaw::value((double)g0[c0], (double)g0[c1], (double)g1[c0], (double)g1[c1], wy0, wy1, wx0, wx1);
        }
    }
    const double mean[3] = {m0, m1, m2};
    const size_t plane = (size_t)g.H * g.W;
    const size_t px = ((size_t)row * g.W + x0) * 3;
    const bool vec = (g.W & 3) == 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int lv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const size_t at = px + 3 * (vec ? j : min(j, g.W - 1 - x0)) + c;
            lv[j] = masked ? ExactLaw::pixel(m[j], (double)probe[at], fill[at]) : (int)probe[at];
        }
        if (U8OUT) {
            uint8_t* o = (uint8_t*)out_any + (size_t)k * 3 * plane + px + c;
            for (int j = 0; j < 4 && x0 + j < g.W; ++j) o[3 * j] = (uint8_t)lv[j];
        } else {
            float* o = (float*)out_any + (size_t)k * 3 * plane + (size_t)row * g.W + x0 + c * plane;
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = ExactLaw::input(lv[j], mean[c]);
            if (vec) {
                *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
                for (int j = 0; j < 4 && x0 + j < g.W; ++j) o[j] = v[j];
            }
        }
    }
}

// parity hook: the float64 masks of a law themselves, n x H x W
template <class Law>
__global__ __launch_bounds__(NT) void strise_masks_kernel(const int* __restrict__ cells, const int* __restrict__ shifts, double* __restrict__ out, StriseGeom g)
{
    __shared__ uint8_t grid[STRISE_MAX_CELLS];
    const int k = blockIdx.y;
    build_grid(grid, cells + (size_t)k * g.n_elem, g.n_elem, g.gh * g.gw);
    const int q = blockIdx.x * NT + threadIdx.x;
    if (q >= g.H * g.W) return;
    const int row = q / g.W, x = q - row * g.W;
    int r0, r1, c0, c1;
    double wy0, wy1, wx0, wx1;
    Law::taps(row + shifts[2 * k], g.gh, g.ry, r0, r1, wy0, wy1);
    Law::taps(x + shifts[2 * k + 1], g.gw, g.rx, c0, c1, wx0, wx1);
    out[(size_t)k * g.H * g.W + q] = Law::value((double)grid[r0 * g.gw + c0], (double)grid[r0 * g.gw + c1], (double)grid[r1 * g.gw + c0],
                                                (double)grid[r1 * g.gw + c1], wy0, wy1, wx0, wx1);
}

// 1 / |v| of a D-vector, by one wavefront (every lane returns it)
__device__ inline double wave_inv_norm(const float* __restrict__ v, int D, int lane)
{
    double acc = 0.0;
    for (int d = lane; d < D; d += 64) acc += (double)v[d] * (double)v[d];
    return 1.0 / sqrt(wave_sum_all(acc));
}

// blackbox.py:385: 1 - 0.5 * | p / |p| - g / |g| |
__device__ inline double wave_similarity(const float* __restrict__ p, double pinv, const float* __restrict__ gv, double ginv, int D, int lane)
{
    double acc = 0.0;
    for (int d = lane; d < D; d += 64) {
        const double t = (double)p[d] * pinv - (double)gv[d] * ginv;
        acc += t * t;
    }
    return 1.0 - 0.5 * sqrt(wave_sum_all(acc));
}

// the unmasked probe against every reference and gallery embedding (blackbox.py:398,403), and 1 / |g| of each: one wavefront per vector
__global__ __launch_bounds__(NT) void strise_orig_kernel(const float* __restrict__ emb0, const float* __restrict__ refs, int n_refs, const float* __restrict__ gal,
                                                         int n_gal, int D, double* __restrict__ orig, double* __restrict__ ginv)
{
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    if (j >= n_refs + n_gal) return;
    const float* gv = j < n_refs ? refs + (size_t)j * D : gal + (size_t)(j - n_refs) * D;
    const double gi = wave_inv_norm(gv, D, lane);
    const double pinv = wave_inv_norm(emb0, D, lane);
    const double sim = wave_similarity(emb0, pinv, gv, gi, D, lane);
    if (lane == 0) { orig[j] = sim; ginv[j] = gi; }
}

// K_strise_score: contrastive triplet similarity (blackbox.py:390-394) of the images [first, first + count) of a batch, one wavefront per mask:
// a wavefront reduction over D per (mask, reference | gallery image), then the mean over the broadcast pairs
__global__ __launch_bounds__(NT) void strise_score_kernel(const float* __restrict__ emb, int first, int count, const float* __restrict__ refs, int n_refs,
                                                          const float* __restrict__ gal, int n_gal, int D, const double* __restrict__ orig,
                                                          const double* __restrict__ ginv, double* __restrict__ scores)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    if (i >= count) return;
    const float* p = emb + (size_t)(first + i) * D;
    const double pinv = wave_inv_norm(p, D, lane);
    const int J = max(n_refs, n_gal);
    // a lone reference or gallery image is broadcast over the other side (blackbox.py:391-393): its similarity is taken once
    const bool one_ref = n_refs == 1 && J > 1, one_gal = n_gal == 1 && J > 1;
    double sr = one_ref ? wave_similarity(p, pinv, refs, ginv[0], D, lane) : 0.0;
    double sg = one_gal ? wave_similarity(p, pinv, gal, ginv[n_refs], D, lane) : 0.0;
    double acc = 0.0;
    for (int j = 0; j < J; ++j) {
        const int jr = one_ref ? 0 : j, jg = one_gal ? 0 : j;
        if (!one_ref) sr = wave_similarity(p, pinv, refs + (size_t)jr * D, ginv[jr], D, lane);
        if (!one_gal) sg = wave_similarity(p, pinv, gal + (size_t)jg * D, ginv[n_refs + jg], D, lane);
        acc += (orig[jr] - sr) - (orig[n_refs + jg] - sg);
    }
    if (lane == 0) scores[i] = acc / (double)J;
}

// Merge, step 1.  Masks that share a shift share their interpolation weights, and the blend is linear in the grid: per shift, the weighted sum of
// the masks is the blend of  A[cell] = sum of w_k over the masks k that drew the cell  taken from the sum of their weights.  One workgroup per
// shift walks its masks in index order; the cells of one mask are distinct (drawn without replacement), so the adds of one mask do not meet.
__global__ __launch_bounds__(NT) void strise_merge_cells_kernel(const double* __restrict__ weights, const int* __restrict__ cells, const int* __restrict__ order,
                                                                const int* __restrict__ group_off, double* __restrict__ A, double* __restrict__ wsum, StriseGeom g)
{
    __shared__ double acc[STRISE_MAX_CELLS];
    const int grp = blockIdx.x, nc = g.gh * g.gw;
    for (int i = threadIdx.x; i < nc; i += NT) acc[i] = 0.0;
    double total = 0.0;
    __syncthreads();
    for (int m = group_off[grp]; m < group_off[grp + 1]; ++m) {
        const int k = order[m];
        const double w = weights[k];
        if (w == 0.0) continue;
        total += w;
        for (int i = threadIdx.x; i < g.n_elem; i += NT) acc[cells[(size_t)k * g.n_elem + i]] += w;
        __syncthreads();
    }
    for (int i = threadIdx.x; i < nc; i += NT) A[(size_t)grp * nc + i] = acc[i];
    if (threadIdx.x == 0) wsum[grp] = total;
}

// Merge, step 2: per pixel, sum over the shifts of (sum of weights - blend of A), then sign * (1 - sum / count)  (blackbox.py:416-438)
__global__ __launch_bounds__(NT) void strise_merge_pixels_kernel(const double* __restrict__ A, const double* __restrict__ wsum, double count, double sign,
                                                                 double* __restrict__ sal, StriseGeom g)
{
    const int q = blockIdx.x * NT + threadIdx.x;
    if (q >= g.H * g.W) return;
    const int row = q / g.W, x = q - row * g.W, nc = g.gh * g.gw;
    double acc = 0.0;
    for (int sx = 0; sx < g.scale; ++sx) {
        int r0, r1;
        double wy0, wy1;
        ClosedLaw::taps(row + sx, g.gh, g.ry, r0, r1, wy0, wy1);
        for (int sy = 0; sy < g.scale; ++sy) {
            const int grp = sx * g.scale + sy;
            const double ws = wsum[grp];
            if (ws == 0.0) continue;
            int c0, c1;
            double wx0, wx1;
            ClosedLaw::taps(x + sy, g.gw, g.rx, c0, c1, wx0, wx1);
            const double* a = A + (size_t)grp * nc;
            acc += ws - ClosedLaw::value(a[r0 * g.gw + c0], a[r0 * g.gw + c1], a[r1 * g.gw + c0], a[r1 * g.gw + c1], wy0, wy1, wx0, wx1);
        }
    }
    sal[q] = sign * (1.0 - acc / count);
}

// Merge, step 3: min-shift and max-normalise (blackbox.py:440-441), one workgroup, on the wavefront reductions of common.h
__global__ __launch_bounds__(1024) void strise_normalize_kernel(double* __restrict__ sal, int n)
{
    __shared__ double s_mn[16], s_mx[16];
    double mn = INFINITY, mx = -INFINITY;
    for (int i = threadIdx.x; i < n; i += 1024) { const double v = sal[i]; mn = fmin(mn, v); mx = fmax(mx, v); }
    wave_min_max(mn, mx);
    if ((threadIdx.x & 63) == 0) { s_mn[threadIdx.x >> 6] = mn; s_mx[threadIdx.x >> 6] = mx; }
    __syncthreads();
    mn = s_mn[0]; mx = s_mx[0];
    for (int i = 1; i < 16; ++i) { mn = fmin(mn, s_mn[i]); mx = fmax(mx, s_mx[i]); }
    const double top = mx - mn;
    for (int i = threadIdx.x; i < n; i += 1024) sal[i] = (sal[i] - mn) / top;
}

// K_strise_quant_lum: the quantised chain for XFR_U8_LUMINANCE networks (Light-CNN, lightcnn.py:19-31): q at probe resolution, PIL's bilinear
// Resize + CenterCrop as two integer passes from the caller's cropped tap tables (columns first, rounded to uint8, then rows), then rgb2gray as
// u8hwc_to_cnhw_kernel states it, into the 1 x in_h x in_w input.  One workgroup per (image, band of STRISE_LUM_BAND output rows): q of the
// probe rows the band reads as bytes in LDS, the horizontal pass into a second byte plane, the vertical pass and the luminance from there.
// Dynamic LDS: rows_max x (W + in_w) x 3 bytes behind the grid.
__global__ __launch_bounds__(NT) void strise_quant_lum_kernel(const uint8_t* __restrict__ probe, const double* __restrict__ fill, const int* __restrict__ cells,
                                                              const int* __restrict__ shifts, const StriseTap* __restrict__ row_tab,
                                                              const StriseTap* __restrict__ col_tab, float* __restrict__ out, StriseGeom g, int in_h, int in_w,
                                                              int rows_max, double w0, double w1, double w2)
{
    __shared__ uint8_t grid[STRISE_MAX_CELLS];
    extern __shared__ uint8_t planes[];
    uint8_t* qs = planes;                                      // [rows][W][3]
    uint8_t* hs = planes + (size_t)rows_max * g.W * 3;         // [rows][in_w][3]
    const int k = blockIdx.y;
    build_grid(grid, cells + (size_t)k * g.n_elem, g.n_elem, g.gh * g.gw);
    const int oy0 = blockIdx.x * STRISE_LUM_BAND, oy1 = min(oy0 + STRISE_LUM_BAND, in_h);
    int lo = g.H, hi = 0;
    for (int oy = oy0; oy < oy1; ++oy) {
        lo = min(lo, row_tab[oy].first);
        hi = max(hi, row_tab[oy].first + row_tab[oy].count);
    }
    const int rows = min(hi - lo, rows_max);                   // the host sized rows_max by the same walk
    const int sx = shifts[2 * k], sy = shifts[2 * k + 1];
    const bool masked = sx >= 0;
    for (int i = threadIdx.x; i < rows * g.W; i += NT) {
        const int r = i / g.W, x = i - r * g.W;
        const size_t at = ((size_t)(lo + r) * g.W + x) * 3;
        uint8_t* o = qs + (size_t)i * 3;
        if (masked) {
            int r0, r1, c0, c1;
            double wy0, wy1, wx0, wx1;
            ExactLaw::taps(lo + r + sx, g.gh, g.ry, r0, r1, wy0, wy1);
            ExactLaw::taps(x + sy, g.gw, g.rx, c0, c1, wx0, wx1);
            const double m = ExactLaw::value((double)grid[r0 * g.gw + c0], (double)grid[r0 * g.gw + c1], (double)grid[r1 * g.gw + c0],
                                             (double)grid[r1 * g.gw + c1], wy0, wy1, wx0, wx1);
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c] = (uint8_t)ExactLaw::pixel(m, (double)probe[at + c], fill[at + c]);
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c] = probe[at + c];
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < rows * in_w; i += NT) {
        const int r = i / in_w, ox = i - r * in_w;
        const StriseTap& t = col_tab[ox];
        const uint8_t* px = qs + ((size_t)r * g.W + t.first) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) hs[(size_t)i * 3 + c] = (uint8_t)resample_u8(px + c, 3, t);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < (oy1 - oy0) * in_w; i += NT) {
        const int oy = oy0 + i / in_w, ox = i % in_w;
        const StriseTap& t = row_tab[oy];
        const uint8_t* px = hs + ((size_t)(t.first - lo) * in_w + ox) * 3;
        const int r = resample_u8(px, in_w * 3, t), gr = resample_u8(px + 1, in_w * 3, t), b = resample_u8(px + 2, in_w * 3, t);
        // (rgb / 255) @ w, left to right (elementwise.hip, u8hwc_to_cnhw_kernel)
        double v = mul_rn(div_rn((double)r, 255.0), w0);
        v = add_rn(v, mul_rn(div_rn((double)gr, 255.0), w1));
        v = add_rn(v, mul_rn(div_rn((double)b, 255.0), w2));
        out[((size_t)k * in_h + oy) * in_w + ox] = (float)v;
    }
}

}  // namespace

// the grid of the kernels that take four pixels of a row per thread and one image per blockIdx.y
static dim3 quad_grid(const StriseGeom& g, int n) { return dim3((g.H * ((g.W + 3) / 4) + NT - 1) / NT, n); }

void launch_strise_masked(const uint8_t* probe, const double* fill, const int* cells, const int* shifts, int n, float* out, const StriseGeom& g,
                          const double* mean, hipStream_t s)
{
    hipLaunchKernelGGL(strise_masked_kernel, quad_grid(g, n), dim3(NT), 0, s, probe, fill, cells, shifts, out, g, mean[0], mean[1], mean[2]);
}

void launch_strise_quant(const uint8_t* probe, const double* fill, const int* cells, const int* shifts, int n, float* out, const StriseGeom& g,
                         const double* mean, hipStream_t s)
{
    hipLaunchKernelGGL(strise_quant_kernel<false>, quad_grid(g, n), dim3(NT), 0, s, probe, fill, cells, shifts, (void*)out, g, mean[0], mean[1], mean[2]);
}

void launch_strise_quant_u8(const uint8_t* probe, const double* fill, const int* cells, const int* shifts, int n, uint8_t* out, const StriseGeom& g, hipStream_t s)
{
    hipLaunchKernelGGL(strise_quant_kernel<true>, quad_grid(g, n), dim3(NT), 0, s, probe, fill, cells, shifts, (void*)out, g, 0.0, 0.0, 0.0);
}

void launch_strise_masks(const int* cells, const int* shifts, int n, bool exact, double* out, const StriseGeom& g, hipStream_t s)
{
    const dim3 grid((g.H * g.W + NT - 1) / NT, n);
    if (exact) hipLaunchKernelGGL(strise_masks_kernel<ExactLaw>, grid, dim3(NT), 0, s, cells, shifts, out, g);
    else hipLaunchKernelGGL(strise_masks_kernel<ClosedLaw>, grid, dim3(NT), 0, s, cells, shifts, out, g);
}

void launch_strise_quant_lum(const uint8_t* probe, const double* fill, const int* cells, const int* shifts, int n, const StriseTap* row_tab,
                             const StriseTap* col_tab, float* out, const StriseGeom& g, int in_h, int in_w, int rows_max, const double* weight, hipStream_t s)
{
    const size_t lds = strise_lum_lds_bytes(rows_max, g.W, in_w);
    hipLaunchKernelGGL(strise_quant_lum_kernel, dim3((in_h + STRISE_LUM_BAND - 1) / STRISE_LUM_BAND, n), dim3(NT), lds, s, probe, fill, cells, shifts, row_tab,
                       col_tab, out, g, in_h, in_w, rows_max, weight[0], weight[1], weight[2]);
}

void launch_strise_orig(const float* emb0, const float* refs, int n_refs, const float* gal, int n_gal, int D, double* orig, double* ginv, hipStream_t s)
{
    const int per = NT / 64;
    hipLaunchKernelGGL(strise_orig_kernel, dim3((n_refs + n_gal + per - 1) / per), dim3(NT), 0, s, emb0, refs, n_refs, gal, n_gal, D, orig, ginv);
}

void launch_strise_score(const float* emb, int first, int count, const float* refs, int n_refs, const float* gal, int n_gal, int D, const double* orig,
                         const double* ginv, double* scores, hipStream_t s)
{
    if (count < 1) return;
    const int per = NT / 64;
    hipLaunchKernelGGL(strise_score_kernel, dim3((count + per - 1) / per), dim3(NT), 0, s, emb, first, count, refs, n_refs, gal, n_gal, D, orig, ginv, scores);
}

void launch_strise_merge(const double* weights, const int* cells, const int* order, const int* group_off, double* A, double* wsum, double count, double sign,
                         double* sal, const StriseGeom& g, hipStream_t s)
{
    hipLaunchKernelGGL(strise_merge_cells_kernel, dim3(g.scale * g.scale), dim3(NT), 0, s, weights, cells, order, group_off, A, wsum, g);
    hipLaunchKernelGGL(strise_merge_pixels_kernel, dim3((g.H * g.W + NT - 1) / NT), dim3(NT), 0, s, A, wsum, count, sign, sal, g);
    hipLaunchKernelGGL(strise_normalize_kernel, dim3(1), dim3(1024), 0, s, sal, g.H * g.W);
}
