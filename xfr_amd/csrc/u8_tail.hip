// u8_tail.hip -- _mwp_to_saliency of ebp_version != 6 (whitebox.py:451-454) on the device: min-max stretch to uint8 levels, Pillow's
// GaussianBlur(radius=2) of an 'L' image, min-max stretch to uint8 again.  One workgroup per map, the whole chain out of LDS in one launch:
//   stage A   float32 maps: level = (uint8)(255.0f * ((v - mn) / (float32(eps) + (mx - mn)))), every operation one rounded float32 operation
//             (NumPy 2 keeps the Python floats weak: np.uint8(255*((img-np.min(img))/(self.eps+(np.max(img)-np.min(img))))) stays float32);
//             uint8 levels: the same expression as NumPy evaluates it for a uint8 array, in float64 -- a 256-entry table, built literally
//             (the integer floor(255 v / d) is NOT it: at eps = 1e-12 the identity 0..255 comes back one level lower);
//   blur      Pillow's ImagingGaussianBlur(radius 2, 3 passes) = three extended box passes per axis with box radius 1: weights ww = 4473924 for
//             the three centre pixels, fw = 1677722 for the two at distance 2, edges replicated, (acc + 2^23) >> 24 per pass (acc < 2^32);
//             rows first, then columns, every pass rounded to bytes;
//   stage B   the uint8 form of stage A on the blurred bytes.
// Two byte planes of H x W in LDS, ping-ponged by the six passes with a barrier in between.  In every pass -- the column passes too -- consecutive
// lanes take consecutive x of one row, so a lane group reads consecutive bytes of the rows y-2 .. y+2: up to four lanes share a dword (one address per
// bank, broadcast), no two lanes of a group meet on a bank with different dwords, and no transposed plane is ever stored.
// No atomics, no floating-point reassociation (min and max are exact whatever their order): the bytes are a function of the input bits alone.
#include "common.h"
#include <atomic>
#include <math.h>

namespace {

constexpr int UT = 1024;                       // 16 waves: 12-13 pixels per lane and pass on a 112 x 112 map
constexpr unsigned U8_WW = 4473924u;           // Pillow BoxBlur.c, radius 1 of GaussianBlur(2): ww = 2^24 / (2 * 1.375 + 1) as it rounds it
constexpr unsigned U8_FW = 1677722u;           //                                                 fw = (1.375 - 1) * ww

// min and max of the workgroup's values (every lane hands in its own, identities where it has none), to every lane
template <typename T>
__device__ inline void block_minmax(T& mn, T& mx, T* part)
{
    for (int o = 32; o > 0; o >>= 1) {
        const T a = __shfl_down(mn, o), b = __shfl_down(mx, o);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    __syncthreads();                           // part[] may still be read from the previous reduction
    if ((threadIdx.x & 63) == 0) { part[threadIdx.x >> 6] = mn; part[UT / 64 + (threadIdx.x >> 6)] = mx; }
    __syncthreads();
    mn = part[0];
    mx = part[UT / 64];
    for (int k = 1; k < UT / 64; ++k) {
        const T a = part[k], b = part[UT / 64 + k];
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
}

// lut[v] = np.uint8(255 * ((v - mn) / (eps + (mx - mn)))) for a uint8 array: float64, literally
__device__ inline void build_level_lut(unsigned char* lut, int mn, int mx, double eps)
{
    if (threadIdx.x < 256) {
        const int v = (int)threadIdx.x;
        unsigned char r = 0;
        if (v >= mn && v <= mx) {
            const double den = eps + (double)(mx - mn);
            r = (unsigned char)(int)(255.0 * ((double)(v - mn) / den));
        }
        lut[v] = r;
    }
}

// in_kind 0: float32 maps (in_f); 1: uint8 levels (in_b); 2: levels 0..255 held as floats (in_f).  Output as bytes (out_b) or as floats (out_f).
// in_f / out_f may be the same memory: a workgroup has read its map before it writes it.
__global__ __launch_bounds__(UT) void u8_tail_kernel(const float* in_f, const unsigned char* in_b, unsigned char* out_b, float* out_f, int H, int W,
                                                     int in_kind, float eps_f, double eps_d)
{
    extern __shared__ unsigned char u8_planes[];
    __shared__ float part_f[2 * (UT / 64)];
    __shared__ int part_i[2 * (UT / 64)];
    __shared__ unsigned char lut[256];
    const int HW = H * W;
    const size_t base = (size_t)blockIdx.x * HW;
    unsigned char* a = u8_planes;
    unsigned char* b = u8_planes + HW;

    // stage A
    if (in_kind == 0) {
        const float* p = in_f + base;
        float mn = INFINITY, mx = -INFINITY;
        for (int i = threadIdx.x; i < HW; i += UT) {
            const float v = p[i];
            mn = v < mn ? v : mn;
            mx = v > mx ? v : mx;
        }
        block_minmax(mn, mx, part_f);
        const float den = __fadd_rn(eps_f, __fsub_rn(mx, mn));
        for (int i = threadIdx.x; i < HW; i += UT)
            a[i] = (unsigned char)(int)__fmul_rn(255.0f, __fdiv_rn(__fsub_rn(p[i], mn), den));
    } else {
        int mn = 255, mx = 0;
        for (int i = threadIdx.x; i < HW; i += UT) {
            const int v = in_kind == 1 ? (int)in_b[base + i] : (int)in_f[base + i];
            a[i] = (unsigned char)v;
            mn = v < mn ? v : mn;
            mx = v > mx ? v : mx;
        }
        block_minmax(mn, mx, part_i);
        build_level_lut(lut, mn, mx, eps_d);
        __syncthreads();
        for (int i = threadIdx.x; i < HW; i += UT) a[i] = lut[a[i]];       // a lane rewrites the bytes it wrote
    }
    __syncthreads();

    // the six box passes: 0-2 along rows, 3-5 along columns; n = the line's length, st = the step along it
    for (int pass = 0; pass < 6; ++pass) {
        const bool rows = pass < 3;
        const int n = rows ? W : H, st = rows ? 1 : W;
        for (int i = threadIdx.x; i < HW; i += UT) {
            const int y = i / W, x = i - y * W;
            const int c = rows ? x : y;
            const int m2 = c - 2 < 0 ? 0 : c - 2, m1 = c - 1 < 0 ? 0 : c - 1;
            const int p1 = c + 1 > n - 1 ? n - 1 : c + 1, p2 = c + 2 > n - 1 ? n - 1 : c + 2;
            const unsigned char* line = a + (i - c * st);
            const unsigned inner = (unsigned)line[m1 * st] + (unsigned)line[c * st] + (unsigned)line[p1 * st];
            const unsigned outer = (unsigned)line[m2 * st] + (unsigned)line[p2 * st];
            b[i] = (unsigned char)((U8_WW * inner + U8_FW * outer + (1u << 23)) >> 24);      // <= 4 286 578 688 < 2^32
        }
        __syncthreads();
        unsigned char* t = a; a = b; b = t;
    }

    // stage B
    int mn = 255, mx = 0;
    for (int i = threadIdx.x; i < HW; i += UT) {
        const int v = a[i];
        mn = v < mn ? v : mn;
        mx = v > mx ? v : mx;
    }
    block_minmax(mn, mx, part_i);
    build_level_lut(lut, mn, mx, eps_d);
    __syncthreads();
    if (out_b) {
        for (int i = threadIdx.x; i < HW; i += UT) out_b[base + i] = lut[a[i]];
    } else {
        for (int i = threadIdx.x; i < HW; i += UT) out_f[base + i] = (float)lut[a[i]];
    }
}

}  // namespace

// N maps of H x W (1 <= H * W <= U8_TAIL_MAX_HW, checked by the callers).  Exactly one of in_f / in_b and one of out_b / out_f is given;
// levels_as_float: in_f holds levels 0..255 (the merged map of XFR_SUBTREE_UINT8) and takes the uint8 form of stage A.
void launch_u8_tail(const float* in_f, const unsigned char* in_b, bool levels_as_float, unsigned char* out_b, float* out_f, int N, int H, int W,
                    float eps, hipStream_t s)
{
    const size_t lds = 2 * (size_t)H * W;
    if (lds > 48 * 1024) {      // once per device: above the default limit of dynamic LDS
        static std::atomic<unsigned long long> done{0ull};
        int dev = 0;
        (void)hipGetDevice(&dev);
        const unsigned long long bit = 1ull << (dev & 63);
        if (!(done.load(std::memory_order_relaxed) & bit)) {
            (void)hipFuncSetAttribute((const void*)u8_tail_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * U8_TAIL_MAX_HW);
            done.fetch_or(bit);
        }
    }
    const int kind = in_b ? 1 : (levels_as_float ? 2 : 0);
    hipLaunchKernelGGL(u8_tail_kernel, dim3(N), dim3(UT), lds, s, in_f, in_b, out_b, out_f, H, W, kind, eps, (double)eps);
}
