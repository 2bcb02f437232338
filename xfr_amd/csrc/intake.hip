// intake.hip -- image intake on the device: what stands between a decoded uint8 crop and the network-size uint8 batch of xfr_forward_u8 --
// Whitebox.convert_from_numpy (python/xfr/models/whitebox.py:787-806) behind xfr.utils.image_loader (python/xfr/utils.py:39-202): the / 255 head,
// skimage's order-1 resize as saliency_io.resize_linear restates it (a Gaussian pre-filter on the shrinking axes, scipy.ndimage.zoom(order=1,
// mode='mirror', grid_mode=True), the clip to the crop's range), the truncation to bytes, and, for Light-CNN, Pillow's integer bilinear
// Resize + CenterCrop from the caller's tap tables.  Float64 throughout, plain VALU.  The law, per crop u of h x w x C and an output of H x W:
//     head        a = (double)u / 255.0 (F64) or (double)((float)u / 255.0f) (F32); 256 values, a table in LDS
//     pre-filter  axis 0 then axis 1, each only with sigma = (f - 1) / 2 > 1e-15, f = h / H or w / W: radius r = int(4 sigma + 0.5), weights
//                 w[0 .. r] from the host (w[r] the centre), out[l] = a[l] w[r], then for ii = -r .. -1: out[l] += (a[l + ii] + a[l - ii]) w[r + ii],
//                 indices folded with period 2 (n - 1) (mirror, the edge not repeated), a line of one value constant
//     zoom        per axis cc = (o + 0.5) (n / m) - 0.5, c = |cc|, st = floor(c), w0 = 1 - (c - st), w1 = 1 - w0, taps st and st + 1, the second
//                 folded the same way; the pixel is (((0 + (G00 wy0) wx0) + (G01 wy0) wx1) + (G10 wy1) wx0) + (G11 wy1) wx1
//     clip        to [min a, max a] over all C channels of the crop; byte = uint8(v * 255.0), truncated
//     same size   no resize: uint8(a * 255.0), in float32 up to the truncation under the F32 head
// One thread computes one element and no sum crosses threads: a crop's bytes depend on the crop alone, not on the batch, its place in it or the
// launch.  The pre-filter's planes (h x w x C doubles per crop) are a workspace in global memory.  Contraction is off for the whole file: every
// product and sum below is one rounded operation, and the truncation reads the last bit.
// The host side (argument checks, the chunks, the weights, the staging of host sources) is intake_abi.hip.
#include "common.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;

// index i of a line of n values extended by mirroring without repeating the edge
__device__ inline int fold_mirror(int i, int n)
{
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    i %= p;
    if (i < 0) i += p;
    return i >= n ? p - i : i;
}

// the head of byte u: the quotient of two float32 values formed in float64 and rounded once is the correctly rounded float32 quotient
__device__ inline double head_value(int u, int head)
{
    const double q = (double)u / 255.0;
    return head == INTAKE_HEAD_F32 ? (double)(float)q : q;
}

// ---- K_intake_range: one workgroup per crop: the heads of its least and largest byte (the head is monotone) ---------------------------------
__global__ __launch_bounds__(NT) void intake_range_kernel(const uint8_t* __restrict__ src, const IntakeItem* __restrict__ items, double* __restrict__ lohi)
{
    __shared__ int s_mn[NT / 64], s_mx[NT / 64];
    const IntakeItem it = items[blockIdx.x];
    const int wc = it.w * it.C;
    int mn = 255, mx = 0;
    for (int y = 0; y < it.h; ++y) {
        const uint8_t* row = src + it.src + (long)y * it.stride;
        for (int x = threadIdx.x; x < wc; x += NT) { const int v = row[x]; mn = min(mn, v); mx = max(mx, v); }
    }
    for (int d = 32; d > 0; d >>= 1) { mn = min(mn, __shfl_down(mn, d)); mx = max(mx, __shfl_down(mx, d)); }
    if ((threadIdx.x & 63) == 0) { s_mn[threadIdx.x >> 6] = mn; s_mx[threadIdx.x >> 6] = mx; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int i = 1; i < NT / 64; ++i) { mn = min(mn, s_mn[i]); mx = max(mx, s_mx[i]); }
    lohi[2 * (size_t)blockIdx.x] = head_value(mn, it.head);
    lohi[2 * (size_t)blockIdx.x + 1] = head_value(mx, it.head);
}

// ---- K_intake_gauss: one thread per element (y, x, c) of a crop: one pass of the pre-filter ---------------------------------------------------
// pass 0: axis 0 from the bytes into plane A (ry > 0); pass 1: axis 1 from the bytes into A (ry == 0 < rx); pass 2: axis 1 from A into B (both)
__global__ __launch_bounds__(NT) void intake_gauss_kernel(const uint8_t* __restrict__ src, const IntakeItem* __restrict__ items, const double* __restrict__ wts,
                                                          const double* __restrict__ in, double* __restrict__ out, int pass)
{
    __shared__ double s_head[256];
    const IntakeItem it = items[blockIdx.y];
    const bool mine = pass == 0 ? it.ry > 0 : pass == 1 ? (it.ry == 0 && it.rx > 0) : (it.ry > 0 && it.rx > 0);
    const long n_el = (long)it.h * it.w * it.C;
    if (!mine || (long)blockIdx.x * NT >= n_el) return;                  // the whole workgroup leaves
    const bool from_u8 = pass != 2;
    if (from_u8) {
        s_head[threadIdx.x] = head_value(threadIdx.x, it.head);
        __syncthreads();
    }
    const long e = (long)blockIdx.x * NT + threadIdx.x;
    if (e >= n_el) return;
    const int axis = pass == 0 ? 0 : 1;
    const int wc = it.w * it.C;
    const int y = (int)(e / wc), xc = (int)(e - (long)y * wc), c = xc % it.C;
    const int r = axis == 0 ? it.ry : it.rx, n = axis == 0 ? it.h : it.w, l = axis == 0 ? y : xc / it.C;
    const double* w = wts + ((size_t)blockIdx.y * 2 + axis) * INTAKE_WEIGHTS;
    const uint8_t* u = src + it.src;
    const double* a = in + it.ws;
    auto at = [&](int j) -> double {
        if (from_u8) return s_head[u[axis == 0 ? (long)j * it.stride + xc : (long)y * it.stride + j * it.C + c]];
        return a[axis == 0 ? (long)j * wc + xc : (long)y * wc + j * it.C + c];
    };
    double acc = at(l) * w[r];
    const bool inside = l - r >= 0 && l + r < n;
    for (int ii = -r; ii < 0; ++ii) {
        const int ja = inside ? l + ii : fold_mirror(l + ii, n), jb = inside ? l - ii : fold_mirror(l - ii, n);
        acc += (at(ja) + at(jb)) * w[r + ii];
    }
    out[it.ws + e] = acc;
}

// the two taps of output index o of an axis of n values: indices inside [0, n) whatever the arithmetic does
__device__ inline void zoom_taps(int o, double scale, int n, int& i0, int& i1, double& w0, double& w1)
{
    const double cc = ((double)o + 0.5) * scale - 0.5;
    double c = cc < 0.0 ? -cc : cc;
    if (n == 1) c = 0.0;
    const double st = floor(c);
    w0 = 1.0 - (c - st);
    w1 = 1.0 - w0;
    i0 = min(max((int)st, 0), n - 1);
    i1 = fold_mirror(i0 + 1, n);
}

// ---- K_intake_zoom: one thread per output pixel, its three bytes -----------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void intake_zoom_kernel(const uint8_t* __restrict__ src, const IntakeItem* __restrict__ items, const double* __restrict__ lohi,
                                                         const double* __restrict__ plane_a, const double* __restrict__ plane_b, int H, int W,
                                                         uint8_t* __restrict__ out)
{
    __shared__ double s_head[256];
    const IntakeItem it = items[blockIdx.y];
    s_head[threadIdx.x] = head_value(threadIdx.x, it.head);
    __syncthreads();
    const long p = (long)blockIdx.x * NT + threadIdx.x;
    if (p >= (long)H * W) return;
    uint8_t* o = out + ((size_t)blockIdx.y * H * W + p) * 3;
    const uint8_t* u = src + it.src;
    const int oy = (int)(p / W), ox = (int)(p - (long)oy * W);
    uint8_t b[3];
    if (it.identity) {                                                    // h x w == H x W
        for (int ch = 0; ch < 3; ++ch) {
            const int v = u[(long)oy * it.stride + ox * it.C + (it.C == 1 ? 0 : ch)];
            if (it.head == INTAKE_HEAD_F32) {
                const float a = (float)((double)v / 255.0);
                b[ch] = (uint8_t)(int)(float)((double)a * 255.0);         // a float32 product: 32 significant bits, exact in float64, rounded once
            } else {
                b[ch] = (uint8_t)(int)(s_head[v] * 255.0);
            }
        }
    } else {
        int y0, y1, x0, x1;
        double wy0, wy1, wx0, wx1;
        zoom_taps(oy, it.sy, it.h, y0, y1, wy0, wy1);
        zoom_taps(ox, it.sx, it.w, x0, x1, wx0, wx1);
        const double lo = lohi[2 * (size_t)blockIdx.y], hi = lohi[2 * (size_t)blockIdx.y + 1];
        const double* a = (it.zoom_from == INTAKE_FROM_B ? plane_b : plane_a) + it.ws;
        const int wc = it.w * it.C;
        const int nch = it.C == 1 ? 1 : 3;
        for (int ch = 0; ch < nch; ++ch) {
            double g00, g01, g10, g11;
            if (it.zoom_from == INTAKE_FROM_U8) {
                g00 = s_head[u[(long)y0 * it.stride + x0 * it.C + ch]];
                g01 = s_head[u[(long)y0 * it.stride + x1 * it.C + ch]];
                g10 = s_head[u[(long)y1 * it.stride + x0 * it.C + ch]];
                g11 = s_head[u[(long)y1 * it.stride + x1 * it.C + ch]];
            } else {
                g00 = a[(long)y0 * wc + x0 * it.C + ch];
                g01 = a[(long)y0 * wc + x1 * it.C + ch];
                g10 = a[(long)y1 * wc + x0 * it.C + ch];
                g11 = a[(long)y1 * wc + x1 * it.C + ch];
            }
            double t = 0.0;
            t += (g00 * wy0) * wx0;
            t += (g01 * wy0) * wx1;
            t += (g10 * wy1) * wx0;
            t += (g11 * wy1) * wx1;
            t = fmin(fmax(t, lo), hi);
            b[ch] = (uint8_t)(int)(t * 255.0);
        }
        if (nch == 1) b[1] = b[2] = b[0];
    }
    o[0] = b[0];
    o[1] = b[1];
    o[2] = b[2];
}

// ---- K_intake_taps: one pass of Pillow's 8-bit resampling over the three channels, one thread per output byte ---------------------------------
// horizontal: in [n][H][W][3] -> out [n][H][m][3] by tab [m]; vertical: in [n][H][W][3] -> out [n][m][W][3]
__global__ __launch_bounds__(NT) void intake_taps_kernel(const uint8_t* __restrict__ in, int H, int W, const StriseTap* __restrict__ tab, int m, int vertical,
                                                         uint8_t* __restrict__ out)
{
    const int oh = vertical ? m : H, ow = vertical ? W : m;
    const long p = (long)blockIdx.x * NT + threadIdx.x;
    if (p >= (long)oh * ow * 3) return;
    const int ch = (int)(p % 3);
    const long px = p / 3;
    const int y = (int)(px / ow), x = (int)(px - (long)y * ow);
    const uint8_t* img = in + (size_t)blockIdx.y * H * W * 3;
    const StriseTap& t = tab[vertical ? y : x];
    const uint8_t* first = vertical ? img + ((long)t.first * W + x) * 3 + ch : img + ((long)y * W + t.first) * 3 + ch;
    out[(size_t)blockIdx.y * oh * ow * 3 + p] = (uint8_t)resample_u8(first, vertical ? W * 3 : 3, t);
}

unsigned blocks_of(long n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

void launch_intake_range(const uint8_t* src, const IntakeItem* items, int n, double* lohi, hipStream_t s)
{
    hipLaunchKernelGGL(intake_range_kernel, dim3(n), dim3(NT), 0, s, src, items, lohi);
}

void launch_intake_prefilter(const uint8_t* src, const IntakeItem* items, int n, const double* wts, double* plane_a, double* plane_b, long max_elems, int which,
                             hipStream_t s)
{
    const dim3 grid(blocks_of(max_elems, NT), n);
    if (which & 1) hipLaunchKernelGGL(intake_gauss_kernel, grid, dim3(NT), 0, s, src, items, wts, (const double*)nullptr, plane_a, 0);
    if (which & 2) hipLaunchKernelGGL(intake_gauss_kernel, grid, dim3(NT), 0, s, src, items, wts, (const double*)nullptr, plane_a, 1);
    if (which & 4) hipLaunchKernelGGL(intake_gauss_kernel, grid, dim3(NT), 0, s, src, items, wts, (const double*)plane_a, plane_b, 2);
}

void launch_intake_zoom(const uint8_t* src, const IntakeItem* items, int n, const double* lohi, const double* plane_a, const double* plane_b, int H, int W,
                        uint8_t* out, hipStream_t s)
{
    hipLaunchKernelGGL(intake_zoom_kernel, dim3(blocks_of((long)H * W, NT), n), dim3(NT), 0, s, src, items, lohi, plane_a, plane_b, H, W, out);
}

void launch_intake_taps(const uint8_t* q, int n, int H, int W, const StriseTap* row_tab, const StriseTap* col_tab, int fh, int fw, uint8_t* mid, uint8_t* out,
                        hipStream_t s)
{
    hipLaunchKernelGGL(intake_taps_kernel, dim3(blocks_of((long)H * fw * 3, NT), n), dim3(NT), 0, s, q, H, W, col_tab, fw, 0, mid);
    hipLaunchKernelGGL(intake_taps_kernel, dim3(blocks_of((long)fh * fw * 3, NT), n), dim3(NT), 0, s, (const uint8_t*)mid, H, fw, row_tab, fh, 1, out);
}
