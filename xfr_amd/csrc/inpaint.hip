// inpaint.hip -- the device side of inpainting-game scoring (python/xfr/inpainting_game/inpainting_game.py:12-197): threshold masks of float64
// saliency maps, the hybrid images, their distances to the two gallery means, intersection-over-union counts.
//
// Masks (create_threshold_masks, :26-65).  Per map, in float64:  v = sal + nz * noise * max_noise,  s = v / sum(v);  'percent-density' compares
// cdf / max(cdf) with 1 - p / 100, cdf being the running sum of s in ascending order scattered back to the pixels (:44-53); explicit thresholds
// compare s itself (:57,65).  The thresholds fall as the level rises, so the masks are nested and one byte per pixel holds them all: first_on, the
// first level at which the pixel is on (n_levels: never).
// The ascending order is a stable LSD radix sort of the 64-bit patterns of v (sign-folded, so any finite double orders like its key) with the
// flat index as payload, four bits a pass, passes whose digit is shared by all keys skipped.  v and s = v / sum(v) order alike for a positive
// sum, and sorting v keeps the order independent of how the sum was rounded.  EQUAL KEYS ARE ORDERED BY FLAT INDEX (numpy's quicksort leaves
// their order unspecified, :44).  One workgroup sorts one map: thread t owns the items [t * chunk, (t + 1) * chunk) of the current order, counts
// its digits into its own LDS column, a workgroup scan over (digit, thread) turns the counts into offsets, and the thread scatters its items in
// order -- no atomics on floating point anywhere, every sum has a fixed order: results are bit-reproducible from run to run.
// A caller's total (total_in > 0) replaces the workgroup's sum: s = v / total is then the caller's division bit for bit, which is what lets numpy's
// percentile thresholds ('percent-pixels', :57-62), many of which sit on or one ulp beside an element of s, decide the same pixels here.
//
// Soft-edged masks (mask_blur_sigma, :68-75): mask l of a map, first_on <= l as 0.0 / 1.0, goes through a separable Gaussian in float64, axis 0 then
// axis 1, indices clamped to the edge, the intermediate rounded to float64.  Per output, with w[j] the weight at distance j from the centre of
// 2 r + 1 taps:  t = in[0] * w[0];  for j = r, r - 1, ..., 1:  t += (in[-j] + in[+j]) * w[j]  -- every product and sum rounded, no fused multiply-add.
// That is the order of scipy.ndimage.gaussian_filter(mode='nearest', truncate=4.0) (correlate1d's symmetric branch), so the masks are its masks
// bit for bit when the weights are its weights.  inpaint_soft_blend_kernel fuses the two passes with the blend (float)((1 - m) a + m b): one
// workgroup per (hybrid, 16 x 64 tile); the tile's mask bits with a halo of r go to LDS, the axis-0 pass fills a float64 LDS plane of 16 rows, the
// axis-1 pass reads it along rows (consecutive lanes, consecutive doubles), and the tile's m goes through LDS once more so that every thread
// holds four adjacent pixels for float4 stores.  A level that is not blurred and a padding row skip the passes.
// The host side (argument checks, batching, streams) is inpaint_abi.hip.
#include "common.h"
#include <math.h>

namespace {

constexpr int NT = 256;
constexpr int NS = 512;            // threads of the order-statistics workgroup
constexpr int NW = NS / 64;

__device__ inline unsigned long long key_of(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v + 0.0);      // -0 + 0 = +0: the two zeros are one key
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ inline double value_of(unsigned long long k)
{
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// sum over the workgroup in a fixed order: lanes by shuffle, then the wavefronts one after the other (every thread returns it)
__device__ inline double block_sum(double v, double* s_w)
{
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    for (int w = 0; w < NW; ++w) t += s_w[w];
    return t;
}

// exclusive scans over the workgroup's threads, same fixed order
template <class T>
__device__ inline T block_excl_scan(T v, T* s_w)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    T inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const T up = __shfl_up(inc, o);
        if (lane >= o) inc += up;
    }
    __syncthreads();
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    T base = 0;
    for (int k = 0; k < w; ++k) base += s_w[k];
    return base + inc - v;
}

__device__ inline double noisy(const double* __restrict__ sal, const double* __restrict__ noise, double max_noise, int include_zero, long i)
{
    const double a = sal[i];
    const double nz = noise ? ((include_zero || a != 0.0) ? noise[i] : 0.0) : 0.0;      // :27-32: nonzero_saliency * rand
    return add_rn(a, mul_rn(nz, max_noise));                                            // :34-37, no contraction
}

__global__ __launch_bounds__(NS) void inpaint_masks_kernel(const double* __restrict__ sal_all, const double* __restrict__ noise, double max_noise,
                                                          int include_zero, int density, InpaintLevels lv, long n, char* __restrict__ scratch_all,
                                                          uint8_t* __restrict__ first_on_all, double* __restrict__ cdf_all, double total_in)
{
    __shared__ unsigned cnt[16 * NS];
    __shared__ double s_thr[INPAINT_MAX_LEVELS];
    __shared__ double s_wd[NW];
    __shared__ unsigned s_wu[NW];
    __shared__ unsigned long long s_or, s_and;
    const int t = threadIdx.x;
    const long m = blockIdx.x;
    const double* sal = sal_all + m * n;
    uint8_t* first_on = first_on_all + m * n;
    char* scratch = scratch_all + (size_t)m * inpaint_scratch_bytes(n);
    unsigned long long* key[2] = {reinterpret_cast<unsigned long long*>(scratch), reinterpret_cast<unsigned long long*>(scratch) + n};
    double* run = reinterpret_cast<double*>(scratch) + 2 * n;
    unsigned* idx[2] = {reinterpret_cast<unsigned*>(scratch + (size_t)n * 24), reinterpret_cast<unsigned*>(scratch + (size_t)n * 24) + n};
    const int L = lv.n;
    for (int l = t; l < L; l += NS) s_thr[l] = lv.thr[l];
    if (t == 0) { s_or = 0ull; s_and = ~0ull; }

    double total = total_in;                                                            // the caller's sum (the same for every thread), or
    if (!(total_in > 0.0)) {
        double acc = 0.0;
        for (long i = t; i < n; i += NS) acc += noisy(sal, noise, max_noise, include_zero, i);
        total = block_sum(acc, s_wd);                                                   // :39-41
    }

    double top = 1.0;
    if (density) {
        unsigned long long o = 0ull, a = ~0ull;
        for (long i = t; i < n; i += NS) {
            const unsigned long long k = key_of(noisy(sal, noise, max_noise, include_zero, i));
            key[0][i] = k;
            idx[0][i] = (unsigned)i;
            o |= k;
            a &= k;
        }
        atomicOr(&s_or, o);
        atomicAnd(&s_and, a);
        __syncthreads();
        const unsigned long long varying = s_or ^ s_and;
        const long chunk = (n + NS - 1) / NS;
        const long lo = min(n, t * chunk), hi = min(n, lo + chunk);
        int cur = 0;
        for (int shift = 0; shift < 64; shift += 4) {
            if (((varying >> shift) & 15ull) == 0ull) continue;
            const unsigned long long* ks = key[cur];
            const unsigned* is = idx[cur];
            unsigned long long* kd = key[cur ^ 1];
            unsigned* id = idx[cur ^ 1];
            for (int b = 0; b < 16; ++b) cnt[b * NS + t] = 0u;
            for (long i = lo; i < hi; ++i) cnt[(int)((ks[i] >> shift) & 15ull) * NS + t] += 1u;
            __syncthreads();
            // the counters in (digit, thread) order are the array cnt[0 .. 16 NS): each thread scans 16 consecutive ones
            unsigned loc[16], sum = 0u;
#pragma unroll
            for (int k = 0; k < 16; ++k) { loc[k] = sum; sum += cnt[t * 16 + k]; }
            const unsigned base = block_excl_scan(sum, s_wu);
#pragma unroll
            for (int k = 0; k < 16; ++k) cnt[t * 16 + k] = base + loc[k];
            __syncthreads();
            for (long i = lo; i < hi; ++i) {
                const unsigned long long k = ks[i];
                const unsigned pos = cnt[(int)((k >> shift) & 15ull) * NS + t]++;
                kd[pos] = k;
                id[pos] = is[i];
            }
            __syncthreads();
            cur ^= 1;
        }
        // :45-48: the running sum in ascending order, scattered back
        const unsigned long long* ks = key[cur];
        const unsigned* is = idx[cur];
        double part = 0.0;
        for (long i = lo; i < hi; ++i) part += value_of(ks[i]) / total;
        double r = block_excl_scan(part, s_wd);
        double mx = -INFINITY;
        for (long i = lo; i < hi; ++i) {
            r += value_of(ks[i]) / total;
            run[is[i]] = r;
            mx = fmax(mx, r);
        }
        // :50-52: the maximum of the running sums, in any order (a maximum does not depend on it)
        for (int d = 32; d > 0; d >>= 1) mx = fmax(mx, __shfl_down(mx, d));
        __syncthreads();
        if ((t & 63) == 0) s_wd[t >> 6] = mx;
        __syncthreads();
        top = s_wd[0];
        for (int w = 1; w < NW; ++w) top = fmax(top, s_wd[w]);
    }
    __syncthreads();
    // :65: on where the value exceeds the threshold; the thresholds do not rise with the level, so the first such level decides all later ones
    for (long i = t; i < n; i += NS) {
        const double c = density ? run[i] / top : noisy(sal, noise, max_noise, include_zero, i) / total;
        int l = 0;
        while (l < L && !(c > s_thr[l])) ++l;
        first_on[i] = (uint8_t)l;
        if (cdf_all) cdf_all[m * n + i] = c;
    }
}

// K_inpaint_blend (:114-129): with 0/1 masks (1 - m) * a + m * b in float64 followed by .float() is the select.  One thread: four pixels, all channels.
__global__ __launch_bounds__(NT, 8) void inpaint_blend_kernel(const uint8_t* __restrict__ first_on, const float* __restrict__ orig,
                                                             const float* __restrict__ inp, float* __restrict__ out, int C, long HW, long first, long total,
                                                             int n_levels)
{
    const long q = first + blockIdx.y;
    const long map = q < total ? q / n_levels : 0;
    const int level = q < total ? (int)(q - map * n_levels) : -1;                       // padding: no pixel is on
    const long p0 = ((long)blockIdx.x * NT + threadIdx.x) * 4;
    if (p0 >= HW) return;
    const uint8_t* f = first_on + map * HW + p0;
    float* o = out + (size_t)blockIdx.y * C * HW + p0;
    if ((HW & 3) == 0) {
        const uchar4 fo = *reinterpret_cast<const uchar4*>(f);
        const bool on0 = (int)fo.x <= level, on1 = (int)fo.y <= level, on2 = (int)fo.z <= level, on3 = (int)fo.w <= level;
        for (int c = 0; c < C; ++c) {
            const float4 a = *reinterpret_cast<const float4*>(orig + c * HW + p0);
            const float4 b = *reinterpret_cast<const float4*>(inp + c * HW + p0);
            *reinterpret_cast<float4*>(o + c * HW) = make_float4(on0 ? b.x : a.x, on1 ? b.y : a.y, on2 ? b.z : a.z, on3 ? b.w : a.w);
        }
    } else {
        for (int j = 0; j < 4 && p0 + j < HW; ++j) {
            const bool on = (int)f[j] <= level;
            for (int c = 0; c < C; ++c) o[c * HW + j] = on ? inp[c * HW + p0 + j] : orig[c * HW + p0 + j];
        }
    }
}

// ---- soft-edged masks ------------------------------------------------------------------------------------------------------------------
constexpr int TH = 16, TW = 64;                                    // output tile: 16 rows of 64 pixels, one row per wavefront pass
constexpr int RMAX = INPAINT_MAX_BLUR_RADIUS;
constexpr int SW = TW + 2 * RMAX;                                  // row stride of the mask bytes with their halo
constexpr int PS = SW + 1;                                         // row stride of the float64 plane: odd, so the rows of a column spread over the banks
constexpr int ON_BYTES = (TH + 2 * RMAX) * SW;
static_assert(ON_BYTES >= TH * TW * (int)sizeof(double), "the tile's m reuses the bytes' storage");
static_assert(ON_BYTES + TH * PS * 8 + (RMAX + 1) * 8 < 64 * 1024, "static LDS of the soft kernels");

// The tile (y0, x0) of mask `level` of the map f, blurred with radius r (0: left hard), into s_m [TH][TW].  s_m may share its storage with s_on.
__device__ inline void soft_mask_tile(const uint8_t* __restrict__ f, int H, int W, int level, int r, int y0, int x0, const double* s_half,
                                      unsigned char* s_on, double* s_plane, double* s_m)
{
#pragma clang fp contract(off)
    const int t = threadIdx.x;
    const int ph = TH + 2 * r, pw = TW + 2 * r;
    for (int i = t; i < ph * pw; i += NT) {
        const int py = i / pw, px = i - py * pw;
        const int y = min(max(y0 - r + py, 0), H - 1), x = min(max(x0 - r + px, 0), W - 1);      // mode='nearest'
        s_on[py * SW + px] = (int)f[(long)y * W + x] <= level ? 1 : 0;
    }
    __syncthreads();
    if (r == 0) {
        unsigned char on[TH * TW / NT];
        for (int k = 0; k < TH * TW / NT; ++k) { const int i = t + k * NT; on[k] = s_on[(i / TW) * SW + (i % TW)]; }
        __syncthreads();
        for (int k = 0; k < TH * TW / NT; ++k) s_m[t + k * NT] = (double)on[k];
        __syncthreads();
        return;
    }
    for (int i = t; i < TH * pw; i += NT) {                         // axis 0: a sum of two mask values is 0, 1 or 2, exact in any format
        const int row = i / pw, px = i - row * pw;
        const unsigned char* c = s_on + (row + r) * SW + px;
        double acc = mul_rn((double)c[0], s_half[0]);
        for (int j = r; j >= 1; --j) acc = add_rn(acc, mul_rn((double)((int)c[-j * SW] + (int)c[j * SW]), s_half[j]));
        s_plane[row * PS + px] = acc;
    }
    __syncthreads();
    double m[TH * TW / NT];
    for (int k = 0; k < TH * TW / NT; ++k) {                        // axis 1
        const int i = t + k * NT;
        const double* c = s_plane + (i / TW) * PS + (i % TW) + r;
        double acc = mul_rn(c[0], s_half[0]);
        for (int j = r; j >= 1; --j) acc = add_rn(acc, mul_rn(add_rn(c[-j], c[j]), s_half[j]));
        m[k] = acc;
    }
    for (int k = 0; k < TH * TW / NT; ++k) s_m[t + k * NT] = m[k];  // s_on was last read before the barrier above
    __syncthreads();
}

#define SOFT_TILE_PROLOGUE                                                                                              \
    __shared__ __align__(16) unsigned char s_on[ON_BYTES];                                                              \
    __shared__ double s_plane[TH * PS];                                                                                 \
    __shared__ double s_half[RMAX + 1];                                                                                 \
    double* s_m = reinterpret_cast<double*>(s_on);                                                                      \
    const int tiles_x = (W + TW - 1) / TW;                                                                              \
    const int y0 = ((int)blockIdx.x / tiles_x) * TH, x0 = ((int)blockIdx.x % tiles_x) * TW;                             \
    const int row = threadIdx.x / (TW / 4), y = y0 + row, x = x0 + (threadIdx.x % (TW / 4)) * 4;

// K_inpaint_soft_blend (:68-75, :114-129).  grid (tiles of the image, hybrids of the batch)
__global__ __launch_bounds__(NT) void inpaint_soft_blend_kernel(const uint8_t* __restrict__ first_on, const float* __restrict__ orig,
                                                               const float* __restrict__ inp, float* __restrict__ out, int C, int H, int W, long first,
                                                               long total, int n_levels, InpaintBlur blur)
{
#pragma clang fp contract(off)
    SOFT_TILE_PROLOGUE
    const long HW = (long)H * W;
    const long q = first + blockIdx.y;
    float* o = out + (size_t)blockIdx.y * C * HW + (long)y * W + x;
    const long p = (long)y * W + x;
    if (q >= total) {                                               // padding: the original
        if (y >= H) return;
        for (int j = 0; j < 4 && x + j < W; ++j)
            for (int c = 0; c < C; ++c) o[c * HW + j] = orig[c * HW + p + j];
        return;
    }
    const long map = q / n_levels;
    const int level = (int)(q - map * n_levels);
    const int r = blur.soft[level] ? blur.r : 0;
    for (int j = threadIdx.x; j <= r; j += NT) s_half[j] = blur.half[j];
    soft_mask_tile(first_on + map * HW, H, W, level, r, y0, x0, s_half, s_on, s_plane, s_m);
    if (y >= H || x >= W) return;
    if ((W & 3) == 0) {
        const double2 m01 = *reinterpret_cast<const double2*>(s_m + row * TW + (x - x0));
        const double2 m23 = *reinterpret_cast<const double2*>(s_m + row * TW + (x - x0) + 2);
        const double m[4] = {m01.x, m01.y, m23.x, m23.y};
        for (int c = 0; c < C; ++c) {
            const float4 a4 = *reinterpret_cast<const float4*>(orig + c * HW + p);
            const float4 b4 = *reinterpret_cast<const float4*>(inp + c * HW + p);
            const float a[4] = {a4.x, a4.y, a4.z, a4.w}, b[4] = {b4.x, b4.y, b4.z, b4.w};
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = (float)add_rn(mul_rn(sub_rn(1.0, m[j]), (double)a[j]), mul_rn(m[j], (double)b[j]));
            *reinterpret_cast<float4*>(o + c * HW) = make_float4(v[0], v[1], v[2], v[3]);
        }
    } else {
        for (int j = 0; j < 4 && x + j < W; ++j) {
            const double m = s_m[row * TW + (x - x0) + j];
            for (int c = 0; c < C; ++c)
                o[c * HW + j] = (float)add_rn(mul_rn(sub_rn(1.0, m), (double)orig[c * HW + p + j]), mul_rn(m, (double)inp[c * HW + p + j]));
        }
    }
}

// the parity hook's kernel: the same tile function, the float64 masks themselves
__global__ __launch_bounds__(NT) void inpaint_soft_masks_kernel(const uint8_t* __restrict__ first_on, double* __restrict__ masks, int H, int W, long first,
                                                               int n_levels, InpaintBlur blur)
{
    SOFT_TILE_PROLOGUE
    const long HW = (long)H * W;
    const long q = first + blockIdx.y;
    const long map = q / n_levels;
    const int level = (int)(q - map * n_levels);
    const int r = blur.soft[level] ? blur.r : 0;
    for (int j = threadIdx.x; j <= r; j += NT) s_half[j] = blur.half[j];
    soft_mask_tile(first_on + map * HW, H, W, level, r, y0, x0, s_half, s_on, s_plane, s_m);
    if (y >= H) return;
    for (int j = 0; j < 4 && x + j < W; ++j) masks[(size_t)blockIdx.y * HW + (long)y * W + x + j] = s_m[row * TW + (x - x0) + j];
}

// K_inpaint_dist (:134-140), one wavefront per hybrid, float64 from the fp32 embeddings
__global__ __launch_bounds__(NT) void inpaint_dist_kernel(const float* __restrict__ emb, int count, const float* __restrict__ g_orig,
                                                         const float* __restrict__ g_inp, int D, double* __restrict__ pg, double* __restrict__ pr,
                                                         uint8_t* __restrict__ cls)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    if (i >= count) return;
    const float* e = emb + (size_t)i * D;
    double acc = 0.0;
    for (int d = lane; d < D; d += 64) acc += (double)e[d] * (double)e[d];
    const double nrm = sqrt(wave_sum_all(acc));
    double ar = 0.0, ag = 0.0;
    for (int d = lane; d < D; d += 64) {
        const double u = (double)e[d] / nrm;
        const double dr = u - (double)g_orig[d], dg = u - (double)g_inp[d];
        ar += dr * dr;
        ag += dg * dg;
    }
    const double r = sqrt(wave_sum_all(ar)), g = sqrt(wave_sum_all(ag));
    if (lane == 0) { pr[i] = r; pg[i] = g; cls[i] = g < r ? 1 : 0; }
}

// K_inpaint_iou (:178-192): histograms of first_on inside and outside the ground truth (integer LDS atomics), then their prefix sums
__global__ __launch_bounds__(NT) void inpaint_iou_kernel(const uint8_t* __restrict__ first_on, const uint8_t* __restrict__ gt, long n, int n_levels,
                                                        long long* __restrict__ counts)
{
    __shared__ unsigned hist[2][INPAINT_MAX_LEVELS + 1];
    const long m = blockIdx.x;
    for (int l = threadIdx.x; l < 2 * (INPAINT_MAX_LEVELS + 1); l += NT) (&hist[0][0])[l] = 0u;
    __syncthreads();
    for (long i = threadIdx.x; i < n; i += NT) atomicAdd(&hist[gt[i] ? 1 : 0][first_on[m * n + i]], 1u);
    __syncthreads();
    long long n_gt = 0;
    for (int l = 0; l <= n_levels; ++l) n_gt += hist[1][l];
    for (int l = threadIdx.x; l < n_levels; l += NT) {
        long long in_gt = 0, out_gt = 0;
        for (int k = 0; k <= l; ++k) { in_gt += hist[1][k]; out_gt += hist[0][k]; }
        long long* c = counts + (m * n_levels + l) * 3;
        c[0] = in_gt;
        c[1] = n_gt + out_gt;
        c[2] = out_gt;
    }
}

}  // namespace

void launch_inpaint_masks(const double* sal, const double* noise, double max_noise, int include_zero, int density, const InpaintLevels& lv, int n_maps, long n,
                          void* scratch, uint8_t* first_on, double* cdf, hipStream_t s, double total)
{
    hipLaunchKernelGGL(inpaint_masks_kernel, dim3(n_maps), dim3(NS), 0, s, sal, noise, max_noise, include_zero, density, lv, n, (char*)scratch, first_on, cdf,
                       total);
}

// the soft kernels' grid: (tiles of the image, entries of the list)
static dim3 soft_grid(int H, int W, int rows) { return dim3((unsigned)(((H + TH - 1) / TH) * ((W + TW - 1) / TW)), rows); }

void launch_inpaint_soft_blend(const uint8_t* first_on, const float* orig, const float* inpaint, float* out, int C, int H, int W, long first, int rows, long total,
                               int n_levels, const InpaintBlur& blur, hipStream_t s)
{
    hipLaunchKernelGGL(inpaint_soft_blend_kernel, soft_grid(H, W, rows), dim3(NT), 0, s, first_on, orig, inpaint, out, C, H, W, first, total, n_levels, blur);
}

void launch_inpaint_soft_masks(const uint8_t* first_on, double* masks, int H, int W, long first, int rows, int n_levels, const InpaintBlur& blur, hipStream_t s)
{
    hipLaunchKernelGGL(inpaint_soft_masks_kernel, soft_grid(H, W, rows), dim3(NT), 0, s, first_on, masks, H, W, first, n_levels, blur);
}

void launch_inpaint_blend(const uint8_t* first_on, const float* orig, const float* inpaint, float* out, int C, long HW, long first, int rows, long total,
                          int n_levels, hipStream_t s)
{
    const long quads = (HW + 3) / 4;
    hipLaunchKernelGGL(inpaint_blend_kernel, dim3((unsigned)((quads + NT - 1) / NT), rows), dim3(NT), 0, s, first_on, orig, inpaint, out, C, HW, first, total,
                       n_levels);
}

void launch_inpaint_dist(const float* emb, int count, const float* g_orig, const float* g_inp, int D, double* pg, double* pr, uint8_t* cls, hipStream_t s)
{
    if (count < 1) return;
    const int per = NT / 64;
    hipLaunchKernelGGL(inpaint_dist_kernel, dim3((count + per - 1) / per), dim3(NT), 0, s, emb, count, g_orig, g_inp, D, pg, pr, cls);
}

void launch_inpaint_iou(const uint8_t* first_on, const uint8_t* gt, long n, int n_maps, int n_levels, long long* counts, hipStream_t s)
{
    hipLaunchKernelGGL(inpaint_iou_kernel, dim3(n_maps), dim3(NT), 0, s, first_on, gt, n, n_levels, counts);
}
