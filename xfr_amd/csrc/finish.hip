// finish.hip -- saliency finishing on the device: what create_save_smap (python/xfr/show.py:196-222) does to every generated map before it is stored --
// the float32 min-shift and division by the sum, processSaliency's float64 normalisation and cubic-spline resize to the probe size (show.py:131-137),
// and the jet overlay of blend_saliency_map with its defaults (show.py:46-129).  Float64 throughout except the float32 head; plain VALU, no LDS beyond
// the partials of a workgroup reduction.  The resize is scipy.ndimage.zoom(order=3, mode='grid-constant', cval=0, grid_mode=True) in closed form:
//     pad the normalised map a with FINISH_PAD = 12 zeros on every side;
//     along axis 0, then along axis 1, every line of L values becomes its B-spline coefficients, pole z = sqrt(3) - 2:
//         c *= (1 - z)(1 - 1/z);   c[0] = (c[0] + z^(L-1) c[L-1] + sum_{i=1}^{L-2} z^i (c[i] + z^(L-1) c[L-1-i])) / (1 - z^(2(L-1)));
//         c[i] += z c[i-1] upwards;   c[L-1] = (z c[L-2] + c[L-1]) z / (z^2 - 1);   c[i] = z (c[i+1] - c[i]) downwards;
//     output index o of an axis reads x = (o + 0.5) (dim / out) - 0.5 + 12, f = floor(x), t = x - f, taps f-1 .. f+2 with the cubic B-spline weights
//     (1-t)^3/6, (3t^3 - 6t^2 + 4)/6, (-3t^3 + 3t^2 + 3t + 1)/6, t^3/6; the pixel is the 16-tap tensor product, clipped to [min(a.min, 0), max(a.max, 0)].
// The padded coefficient plane of a map ((h + 24) x (w + 24) doubles, 148 KB at the generator's 112 x 112) is a workspace in global memory: it does not
// fit a workgroup's LDS share at any useful occupancy, and 32 of them stay in L2.  One thread filters one line, so no value is ever summed across
// threads: a map's bits depend on nothing but the map.  Every reduction (minimum, maximum, the float64 sum of the head) runs in one workgroup per map
// in a fixed order.  Contraction is off for the whole file: every product and sum below is one rounded operation.
// The host side (argument checks, the workspace, the uploaded table) is finish_abi.hip.
#include "common.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;
constexpr int LINE_NT = 64;                                // threads (= lines) per workgroup of the two prefilter passes
constexpr double POLE = -0.26794919243112270647;           // sqrt(3) - 2
// per-map statistics, FINISH_STATS doubles: what the head leaves for the kernels behind it, and the finished map's range for the overlay
enum { ST_MIN = 0, ST_TOTAL, ST_SHIFT, ST_DENOM, ST_LO, ST_HI, ST_VMIN, ST_VMAX };
static_assert(ST_VMAX < FINISH_STATS, "the statistics fit their row");

// min and max of a workgroup's values, handed to every thread; partials in a fixed order (both are exact, so the order is for form only)
__device__ inline void block_min_max(double& mn, double& mx, double* s_part)
{
    wave_min_max(mn, mx);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { s_part[2 * (threadIdx.x >> 6)] = mn; s_part[2 * (threadIdx.x >> 6) + 1] = mx; }
    __syncthreads();
    mn = fmin(fmin(s_part[0], s_part[2]), fmin(s_part[4], s_part[6]));
    mx = fmax(fmax(s_part[1], s_part[3]), fmax(s_part[5], s_part[7]));
}

// create_save_smap's float32 head for one value: (m - min) / total, both operations rounded to float32 (the quotient of two float32 values, formed in
// float64 and rounded once, is the correctly rounded float32 quotient: 53 >= 2 * 24 + 2).  A map whose shifted sum is zero -- a constant map -- is the
// all-zero map here; numpy's 0 / 0 makes it NaN.
__device__ inline float head_value(float m, float mn, float total)
{
    const float d = m - mn;
    return total == 0.0f ? 0.0f : (float)((double)d / (double)total);
}

// processSaliency's normalisation of one value of map `st`
__device__ inline double normalised(float m, const double* __restrict__ st)
{
    const double s = (double)head_value(m, (float)st[ST_MIN], (float)st[ST_TOTAL]);
    return (s - st[ST_SHIFT]) / st[ST_DENOM];
}

// ---- K_finish_head: one workgroup per map ---------------------------------------------------------------------------------------------
// Thread t owns pixels t, t + 256, ...; its float64 partial sum, the wavefront's shuffle tree and the four wavefronts in order give the total.
// Rounding is monotone, so the head's and the normalisation's extremes are the images of the map's own minimum and maximum.
__global__ __launch_bounds__(NT) void finish_head_kernel(const float* __restrict__ maps, long n_px, const float* __restrict__ totals, double* __restrict__ stats)
{
    __shared__ double s_part[2 * (NT / 64)];
    const float* m = maps + (size_t)blockIdx.x * n_px;
    double mn = INFINITY, mx = -INFINITY;
    for (long i = threadIdx.x; i < n_px; i += NT) { const double v = (double)m[i]; mn = fmin(mn, v); mx = fmax(mx, v); }
    block_min_max(mn, mx, s_part);
    const float mnf = (float)mn;
    double acc = 0.0;
    for (long i = threadIdx.x; i < n_px; i += NT) acc += (double)(m[i] - mnf);
    acc = wave_sum_all(acc);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x != 0) return;
    const float total = totals ? totals[blockIdx.x] : (float)(((s_part[0] + s_part[1]) + s_part[2]) + s_part[3]);
    const double shift = (double)head_value(mnf, mnf, total);
    const double top = (double)head_value((float)mx, mnf, total) - shift;
    const double denom = top + 1e-9;
    double* st = stats + (size_t)blockIdx.x * FINISH_STATS;
    st[ST_MIN] = mn;
    st[ST_TOTAL] = (double)total;
    st[ST_SHIFT] = shift;
    st[ST_DENOM] = denom;
    st[ST_LO] = fmin((shift - shift) / denom, 0.0);       // _resize_cubic's clip range: [min(a.min, 0), max(a.max, 0)]
    st[ST_HI] = fmax(top / denom, 0.0);
}

// ---- the prefilter of one line, in place: L values `stride` apart; zn = z^(L-1) ---------------------------------------------------------
// The two recursions load eight values ahead of the chain that consumes them.
__device__ inline void spline_line(double* __restrict__ c, int L, size_t stride, double zn)
{
    const double z = POLE;
    const double gain = (1.0 - z) * (1.0 - 1.0 / z);
    for (int i = 0; i < L; ++i) c[i * stride] *= gain;
    double sum = c[0] + zn * c[(size_t)(L - 1) * stride];
    double zi = z;
    for (int i = 1; i <= L - 2; ++i) {
        sum += zi * (c[i * stride] + zn * c[(size_t)(L - 1 - i) * stride]);
        zi *= z;
    }
    double prev = sum / (1.0 - zn * zn);
    c[0] = prev;
    for (int i0 = 1; i0 < L; i0 += 8) {
        double v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = i0 + j < L ? c[(size_t)(i0 + j) * stride] : 0.0;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (i0 + j < L) { prev = v[j] + z * prev; c[(size_t)(i0 + j) * stride] = prev; }
    }
    // prev is c[L-1] of the causal pass
    double next = (z * c[(size_t)(L - 2) * stride] + prev) * z / (z * z - 1.0);
    c[(size_t)(L - 1) * stride] = next;
    for (int i0 = L - 2; i0 >= 0; i0 -= 8) {
        double v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = i0 - j >= 0 ? c[(size_t)(i0 - j) * stride] : 0.0;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (i0 - j >= 0) { next = z * (next - v[j]); c[(size_t)(i0 - j) * stride] = next; }
    }
}

// ---- K_finish_cols: one thread per column of a map's padded plane: the normalised map between the zeros, then the prefilter along axis 0 -------------
__global__ __launch_bounds__(LINE_NT) void finish_cols_kernel(const float* __restrict__ maps, int h, int w, const double* __restrict__ stats,
                                                              double* __restrict__ planes, double zn)
{
    const int Lh = h + 2 * FINISH_PAD, Lw = w + 2 * FINISH_PAD;
    const int j = blockIdx.x * LINE_NT + threadIdx.x;
    if (j >= Lw) return;
    const float* m = maps + (size_t)blockIdx.y * h * w;
    const double* st = stats + (size_t)blockIdx.y * FINISH_STATS;
    double* c = planes + (size_t)blockIdx.y * Lh * Lw + j;
    const bool inside = j >= FINISH_PAD && j < FINISH_PAD + w;
    for (int i = 0; i < Lh; ++i) {
        const bool in = inside && i >= FINISH_PAD && i < FINISH_PAD + h;
        c[(size_t)i * Lw] = in ? normalised(m[(size_t)(i - FINISH_PAD) * w + (j - FINISH_PAD)], st) : 0.0;
    }
    if (inside) spline_line(c, Lh, (size_t)Lw, zn);       // a column of zeros stays one
}

// ---- K_finish_rows: one thread per row of the plane: the prefilter along axis 1 ------------------------------------------------------------
__global__ __launch_bounds__(LINE_NT) void finish_rows_kernel(int h, int w, double* __restrict__ planes, double zn)
{
    const int Lh = h + 2 * FINISH_PAD, Lw = w + 2 * FINISH_PAD;
    const int i = blockIdx.x * LINE_NT + threadIdx.x;
    if (i >= Lh) return;
    spline_line(planes + ((size_t)blockIdx.y * Lh + i) * Lw, Lw, 1, zn);
}

// the four taps of output index o: the first tap's index in the padded line and the cubic B-spline weights
__device__ inline int spline_taps(int o, double scale, int dim, double wt[4])
{
    const double x = (((double)o + 0.5) * scale - 0.5) + (double)FINISH_PAD;
    const double f = floor(x);
    const double t = x - f, u = 1.0 - t;
    wt[0] = u * u * u / 6.0;
    wt[1] = (3.0 * t * t * t - 6.0 * t * t + 4.0) / 6.0;
    wt[2] = (-3.0 * t * t * t + 3.0 * t * t + 3.0 * t + 1.0) / 6.0;
    wt[3] = t * t * t / 6.0;
    // out >= dim puts f in [FINISH_PAD - 1, dim + FINISH_PAD - 1]; the clamp keeps the reads inside the plane whatever the arithmetic does
    return min(max((int)f - 1, 0), dim + 2 * FINISH_PAD - 4);
}

// ---- K_finish_resize: one thread per output pixel ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void finish_resize_kernel(const double* __restrict__ planes, int h, int w, int H, int W, double sy, double sx,
                                                           const double* __restrict__ stats, double* __restrict__ sal)
{
    const long p = (long)blockIdx.x * NT + threadIdx.x;
    if (p >= (long)H * W) return;
    const int oy = (int)(p / W), ox = (int)(p - (long)oy * W);
    const int Lh = h + 2 * FINISH_PAD, Lw = w + 2 * FINISH_PAD;
    double wy[4], wx[4];
    const int fy = spline_taps(oy, sy, h, wy), fx = spline_taps(ox, sx, w, wx);
    const double* c = planes + ((size_t)blockIdx.y * Lh + fy) * Lw + fx;
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double* r = c + (size_t)i * Lw;
        const double row = ((wx[0] * r[0] + wx[1] * r[1]) + wx[2] * r[2]) + wx[3] * r[3];
        acc += wy[i] * row;
    }
    const double* st = stats + (size_t)blockIdx.y * FINISH_STATS;
    sal[(size_t)blockIdx.y * H * W + p] = fmin(fmax(acc, st[ST_LO]), st[ST_HI]);
}

// ---- K_finish_identity: the probe's size is the map's: the normalised map itself (_resize_cubic returns its input) ---------------------------
__global__ __launch_bounds__(NT) void finish_identity_kernel(const float* __restrict__ maps, long n_px, const double* __restrict__ stats, double* __restrict__ sal)
{
    const long p = (long)blockIdx.x * NT + threadIdx.x;
    if (p >= n_px) return;
    sal[(size_t)blockIdx.y * n_px + p] = normalised(maps[(size_t)blockIdx.y * n_px + p], stats + (size_t)blockIdx.y * FINISH_STATS);
}

// ---- K_finish_range: one workgroup per finished map: its minimum and maximum, for the overlay ------------------------------------------------
__global__ __launch_bounds__(NT) void finish_range_kernel(const double* __restrict__ sal, long n_px, double* __restrict__ stats)
{
    __shared__ double s_part[2 * (NT / 64)];
    const double* v = sal + (size_t)blockIdx.x * n_px;
    double mn = INFINITY, mx = -INFINITY;
    for (long i = threadIdx.x; i < n_px; i += NT) { mn = fmin(mn, v[i]); mx = fmax(mx, v[i]); }
    block_min_max(mn, mx, s_part);
    if (threadIdx.x == 0) { stats[(size_t)blockIdx.x * FINISH_STATS + ST_VMIN] = mn; stats[(size_t)blockIdx.x * FINISH_STATS + ST_VMAX] = mx; }
}

// ---- K_finish_overlay: one thread per pixel, three channels (blend_saliency_map with its defaults, then create_save_smap's uint8) ------------------
__global__ __launch_bounds__(NT) void finish_overlay_kernel(const double* __restrict__ sal, const uint8_t* __restrict__ probes, long n_px,
                                                            const double* __restrict__ stats, const double* __restrict__ lut, uint8_t* __restrict__ out)
{
    const long p = (long)blockIdx.x * NT + threadIdx.x;
    if (p >= n_px) return;
    const double* st = stats + (size_t)blockIdx.y * FINISH_STATS;
    const size_t q = (size_t)blockIdx.y * n_px + p;
    const double top = st[ST_VMAX] - st[ST_VMIN];
    double alpha = 0.0;
    int idx = 0;
    const bool blend = top > 0.0;                          // else the suppressed map: the image itself (show.py:110-111,127-128)
    if (blend) {
        const double att = (sal[q] - st[ST_VMIN]) / top;
        alpha = pow(fmax(att, 0.0), 0.8);
        idx = att >= 1.0 ? 255 : min(max((int)(att * 256.0), 0), 255);
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const double img = (double)probes[q * 3 + ch] / 255.0;
        const double o = blend ? (1.0 - alpha) * img + alpha * lut[idx * 3 + ch] : img;
        out[q * 3 + ch] = (uint8_t)(fmin(fmax(o, 0.0), 1.0) * 255.0);
    }
}

unsigned blocks_of(long n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

void launch_finish_head(const float* maps, int n, long n_px, const float* totals, double* stats, hipStream_t s)
{
    hipLaunchKernelGGL(finish_head_kernel, dim3(n), dim3(NT), 0, s, maps, n_px, totals, stats);
}

void launch_finish_prefilter(const float* maps, int n, int h, int w, const double* stats, double* planes, hipStream_t s)
{
    const int Lh = h + 2 * FINISH_PAD, Lw = w + 2 * FINISH_PAD;
    hipLaunchKernelGGL(finish_cols_kernel, dim3(blocks_of(Lw, LINE_NT), n), dim3(LINE_NT), 0, s, maps, h, w, stats, planes, pow(POLE, (double)(Lh - 1)));
    hipLaunchKernelGGL(finish_rows_kernel, dim3(blocks_of(Lh, LINE_NT), n), dim3(LINE_NT), 0, s, h, w, planes, pow(POLE, (double)(Lw - 1)));
}

void launch_finish_resize(const double* planes, int n, int h, int w, int H, int W, const double* stats, double* sal, hipStream_t s)
{
    hipLaunchKernelGGL(finish_resize_kernel, dim3(blocks_of((long)H * W, NT), n), dim3(NT), 0, s, planes, h, w, H, W, (double)h / (double)H,
                       (double)w / (double)W, stats, sal);
}

void launch_finish_identity(const float* maps, int n, long n_px, const double* stats, double* sal, hipStream_t s)
{
    hipLaunchKernelGGL(finish_identity_kernel, dim3(blocks_of(n_px, NT), n), dim3(NT), 0, s, maps, n_px, stats, sal);
}

void launch_finish_overlay(const double* sal, const uint8_t* probes, int n, long n_px, double* stats, const double* lut, uint8_t* out, hipStream_t s)
{
    hipLaunchKernelGGL(finish_range_kernel, dim3(n), dim3(NT), 0, s, sal, n_px, stats);
    hipLaunchKernelGGL(finish_overlay_kernel, dim3(blocks_of(n_px, NT), n), dim3(NT), 0, s, sal, probes, n_px, stats, lut, out);
}
