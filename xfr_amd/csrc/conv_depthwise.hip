// conv_depthwise.hip -- depthwise launches on the vector ALU, configuration 14: the grouped launches (ConvParams::groups > 1) with one input or one
// output channel per group, min(Ci, Co) == 1 for Ci = Cin / groups, Co = CoutTot / groups.  That is the forward of a depthwise layer with channel
// multiplier m (Ci 1, Co m), its backward-data pass (Ci m, Co 1, K = m kh kw) and the phases of a strided one.  The contract is launch_conv_group's
// field by field (common.h, both launchers open with grouped_launch_contract_ok): the per-group packs through group_pack_index (one row block, K ordered (ci, kh, kw)), one or two halves (W and relu(W)
// from the same staging into out0 / out1 with bias / bias_pos), relu_in, stride, pad, pad_dw, the batch prefix (NB <= in_nb, out_nb), accumulate and
// the scattered store (out_stride, out_H, out_W, a pre-offset out0).  On the MFMA kernel such a group fills one of 16 rows of a row block and fetches
// every X element once per tap; here a few FLOPs per byte run as plain fp32 FMAs next to the loads.
//
// Caps (everything else returns false and stays on configuration 13): max(Ci, Co) <= 8 -- a thread keeps 2 halves x Co x 4 accumulators, 64 registers
// at Co 8 -- and kh, kw <= 7, so the weights of a group are at most 2 x 8 x 49 floats of LDS; a tile of 128 outputs must stage within 52 KiB of LDS
// (any map of MobileNet size does), and a tile's input span stays under 2^22 elements (the index decode below divides in fp32).
//
// Tile: a workgroup owns one group and TM = 1024 (512, 256, 128 where LDS asks for it) consecutive outputs m of that group's M = NB OH OW, four per
// thread.  In channel-major layout ([C][NB][H][W]) these are whole output rows of consecutive images of one channel: a 7 x 7 stage puts 20 images
// into a tile, a 112 x 112 stage nine rows.  The input the tile needs is one contiguous span of each of the group's Ci channels: it is staged into
// LDS ONCE, 16 bytes a load where W % 4 == 0 and the pointer is aligned (a scalar path otherwise), relu_in applied there.  Every image of the tile
// has its own slab of staged rows, zero-filled first: padding rows and columns, and rows no output reaches, are exact zeros that were never loaded,
// and a tap never reads a neighbouring image.  Every tap of every output, all Co channels and both halves read that staging.
//
// Arithmetic: fp32 FMAs, no MFMA, no atomics.  One output is acc = 0; acc = fma(w[k], x[k], acc) for k = 0 .. K - 1 ascending in the pack's order
// (ci, kh, kw); then + bias; then + the old value where the launch accumulates.  Two launches give the same bits.  They are NOT the bits of
// configuration 13, which sums the same products four k apart in the MFMA's order.  A non-finite input stays in its own image and channel: no other
// output ever multiplies it.
//
// Outputs: where OW % 4 == 0 a thread owns four neighbouring pixels of a row and stores 16 bytes where the output is dense and aligned; otherwise the
// four outputs of a thread are a workgroup apart (m, m + T, ...) and lanes store neighbouring floats.
#include "common.h"

#include <atomic>

namespace {

constexpr int MAX_CH = 8;             // max(Ci, Co)
constexpr int MAX_TAP = 7;            // kh, kw
constexpr int X_FLOATS = 13312;       // LDS staging of X, 52 KiB
constexpr int SPAN_MAX = 1 << 22;     // a tile's input span and output span in elements: exact in the fp32 index decode

typedef float f32x4 __attribute__((ext_vector_type(4)));

std::atomic<long> g_launches{0};
thread_local int g_last_tile = 0;     // TM of this thread's last launch_conv_depthwise that launched (conv_depthwise_last_tile)

struct DwArgs {
    const float *in, *w, *w_pos, *bias, *bias_pos;
    float *out0, *out1;
    int H, W, in_nb, out_nb, kh, kw, stride, pad, padw, OH, OW, K, Kp, M, relu_in, accumulate, out_H, out_W, out_stride;
    int Ci, Co, TM, Wp, SRfull, rows_cap, ws_floats, vec_in;
    float r_ohw, r_OW, r_HW, r_W;
};

// x / d and the remainder for 0 <= x < 2^22, rd = 1.f / d: the fp32 quotient is off by at most one
__device__ __forceinline__ int div_small(int x, int d, float rd, int& rem)
{
    int q = (int)((float)x * rd);
    int r = x - q * d;
    if (r < 0) { --q; r += d; }
    if (r >= d) { ++q; r -= d; }
    rem = r;
    return q;
}

// the images of a tile: image dn (counted from the tile's first) stages the input rows of its output rows [oh_lo, oh_hi] at slab row `srow` on
struct Slabs {
    int nimg, oh_lo0, oh_hiL, rows_first, SRfull, OH, stride, kh, pad;
    __device__ __forceinline__ void of(int dn, int& oh_lo, int& nrows, int& srow) const
    {
        const bool first = dn == 0, last = dn == nimg - 1;
        oh_lo = first ? oh_lo0 : 0;
        const int oh_hi = last ? oh_hiL : OH - 1;
        nrows = (oh_hi - oh_lo) * stride + kh;
        srow = first ? 0 : rows_first + (dn - 1) * SRfull;
    }
};

template <int NH, int CO, bool VEC>
__global__ __launch_bounds__(256) void conv_depthwise_kernel(const DwArgs p)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Ws = smem;                       // [NH][K][CO], columns beyond Co zero
    float* Xs = smem + p.ws_floats;         // [Ci][tot_rows][Wp]
    const int tid = threadIdx.x, nt = blockDim.x;
    const int g = blockIdx.y;
    const int m0 = blockIdx.x * p.TM;
    const int m1 = min(m0 + p.TM, p.M);
    const int ohw = p.OH * p.OW, HW = p.H * p.W, Wp = p.Wp, s = p.stride;
    const int n_first = m0 / ohw, n_last = (m1 - 1) / ohw;
    Slabs sl;
    sl.nimg = n_last - n_first + 1;
    sl.oh_lo0 = (m0 - n_first * ohw) / p.OW;
    sl.oh_hiL = (m1 - 1 - n_last * ohw) / p.OW;
    sl.SRfull = p.SRfull; sl.OH = p.OH; sl.stride = s; sl.kh = p.kh; sl.pad = p.pad;
    sl.rows_first = ((sl.nimg == 1 ? sl.oh_hiL : p.OH - 1) - sl.oh_lo0) * s + p.kh;
    const int rows_last = sl.nimg > 1 ? sl.oh_hiL * s + p.kh : 0;
    const int tot_rows = sl.rows_first + (sl.nimg > 2 ? (sl.nimg - 2) * p.SRfull : 0) + rows_last;
    if (tot_rows > p.rows_cap) return;      // (the launcher sized rows_cap for the worst tile: never taken)
    const int cs = tot_rows * Wp;

    for (int i = tid; i < p.Ci * cs; i += nt) Xs[i] = 0.f;
    for (int i = tid; i < NH * p.K * CO; i += nt) {
        const int co = i % CO, k = (i / CO) % p.K, h = i / (CO * p.K);
        const float* w = h == 0 ? p.w : p.w_pos;
        Ws[i] = co < p.Co ? w[((size_t)g * p.Kp + k) * GROUP_ROWS + co] : 0.f;
    }
    __syncthreads();

    // the staged span of a channel, relative to image n_first: from the first row the first image needs to the last row the last image needs
    {
        const int r_lo = min(max(sl.oh_lo0 * s - p.pad, 0), p.H);
        const int base_last = (sl.nimg > 1 ? 0 : sl.oh_lo0) * s - p.pad;
        const int r_hi = min(max(base_last + (sl.nimg > 1 ? rows_last : sl.rows_first), 0), p.H);
        const int x0 = r_lo * p.W;
        const int cnt = (sl.nimg - 1) * HW + r_hi * p.W - x0;
        for (int ci = 0; ci < p.Ci; ++ci) {
            const float* src = p.in + ((size_t)(g * p.Ci + ci) * p.in_nb + n_first) * HW;
            float* dst = Xs + ci * cs;
            if (p.vec_in) {
                for (int e = 4 * tid; e < cnt; e += 4 * nt) {
                    const int x = x0 + e;
                    f32x4 v = *reinterpret_cast<const f32x4*>(src + x);
                    int rem, col, oh_lo, nrows, srow;
                    const int dn = div_small(x, HW, p.r_HW, rem);
                    const int ih = div_small(rem, p.W, p.r_W, col);
                    sl.of(dn, oh_lo, nrows, srow);
                    const int lr = ih - (oh_lo * s - p.pad);
                    if ((unsigned)lr >= (unsigned)nrows) continue;
                    float* d = dst + (srow + lr) * Wp + col + p.padw;
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if ((unsigned)(col + p.padw + j) < (unsigned)Wp) d[j] = p.relu_in ? fmaxf(v[j], 0.f) : v[j];
                }
            } else {
                for (int e = tid; e < cnt; e += nt) {
                    const int x = x0 + e;
                    const float v = src[x];
                    int rem, col, oh_lo, nrows, srow;
                    const int dn = div_small(x, HW, p.r_HW, rem);
                    const int ih = div_small(rem, p.W, p.r_W, col);
                    sl.of(dn, oh_lo, nrows, srow);
                    const int lr = ih - (oh_lo * s - p.pad);
                    const int lc = col + p.padw;
                    if ((unsigned)lr < (unsigned)nrows && (unsigned)lc < (unsigned)Wp) dst[(srow + lr) * Wp + lc] = p.relu_in ? fmaxf(v, 0.f) : v;
                }
            }
        }
    }
    __syncthreads();

    // this thread's four outputs: their staged top-left corner and their place in the output
    int base[4];
    size_t off[4];
    bool live[4];
    const size_t out_hw = (size_t)p.out_H * p.out_W;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = VEC ? m0 + 4 * tid + i : m0 + tid + nt * i;
        live[i] = m < m1;
        base[i] = 0;
        off[i] = 0;
        if (VEC && i > 0) {                  // OW % 4 == 0: the four are neighbours in one row
            base[i] = base[0] + i * s;
            off[i] = off[0] + (size_t)i * p.out_stride;
        } else if (live[i]) {
            int rem, ow, oh_lo, nrows, srow;
            const int dn = div_small(m - n_first * ohw, ohw, p.r_ohw, rem);
            const int oh = div_small(rem, p.OW, p.r_OW, ow);
            sl.of(dn, oh_lo, nrows, srow);
            base[i] = (srow + (oh - oh_lo) * s) * Wp + ow * s;
            off[i] = (size_t)(n_first + dn) * out_hw + (size_t)oh * p.out_stride * p.out_W + (size_t)ow * p.out_stride;
        }
    }
    if (!live[0]) return;

    float acc[NH][CO][4];
#pragma unroll
    for (int h = 0; h < NH; ++h)
#pragma unroll
        for (int c = 0; c < CO; ++c)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[h][c][i] = 0.f;
    int k = 0;
    for (int ci = 0; ci < p.Ci; ++ci) {
        const float* xc = Xs + ci * cs;
        for (int a = 0; a < p.kh; ++a) {
            const float* xr = xc + a * Wp;
            for (int b = 0; b < p.kw; ++b, ++k) {
                float x[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) x[i] = xr[base[i] + b];
#pragma unroll
                for (int h = 0; h < NH; ++h)
#pragma unroll
                    for (int c = 0; c < CO; ++c) {
                        const float w = Ws[(h * p.K + k) * CO + c];
#pragma unroll
                        for (int i = 0; i < 4; ++i) acc[h][c][i] = fmaf(w, x[i], acc[h][c][i]);
                    }
            }
        }
    }

    const bool dense = p.out_stride == 1 && p.out_H == p.OH && p.out_W == p.OW;
#pragma unroll
    for (int h = 0; h < NH; ++h) {
        float* out = h == 0 ? p.out0 : p.out1;
        const float* bias = h == 0 ? p.bias : p.bias_pos;
        // 16-byte stores: four neighbours of a dense row; OW % 4 == 0 keeps every row's start as aligned as the tensor's
        const bool vec = VEC && dense && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
#pragma unroll
        for (int c = 0; c < CO; ++c) {
            if (c >= p.Co) continue;
            const int co = g * p.Co + c;
            const float bv = bias ? bias[co] : 0.f;
            float* row = out + (size_t)co * p.out_nb * out_hw;
            if (vec) {
                f32x4 v = {acc[h][c][0] + bv, acc[h][c][1] + bv, acc[h][c][2] + bv, acc[h][c][3] + bv};
                f32x4* dst = reinterpret_cast<f32x4*>(row + off[0]);
                if (p.accumulate) { const f32x4 o = *dst; v += o; }
                *dst = v;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (!VEC && !live[i]) continue;
                    float v = acc[h][c][i] + bv;
                    if (p.accumulate) v += row[off[i]];
                    row[off[i]] = v;
                }
            }
        }
    }
}

template <int NH, int CO>
void launch_vec(const DwArgs& a, bool vec, dim3 grid, int threads, size_t lds, hipStream_t s)
{
    if (vec) conv_depthwise_kernel<NH, CO, true><<<grid, threads, lds, s>>>(a);
    else conv_depthwise_kernel<NH, CO, false><<<grid, threads, lds, s>>>(a);
}

template <int CO>
void launch_co(const DwArgs& a, int nhalves, bool vec, dim3 grid, int threads, size_t lds, hipStream_t s)
{
    if (nhalves == 2) launch_vec<2, CO>(a, vec, grid, threads, lds, s);
    else launch_vec<1, CO>(a, vec, grid, threads, lds, s);
}

}  // namespace

long conv_depthwise_launches() { return g_launches.load(); }
int conv_depthwise_last_tile() { return g_last_tile; }

bool launch_conv_depthwise(const ConvParams& p, hipStream_t s)
{
    if (!grouped_launch_contract_ok(p)) return false;
    const int G = p.groups, Ci = p.Cin / G, Co = p.CoutTot / G;
    if ((Ci != 1 && Co != 1) || Ci > MAX_CH || Co > MAX_CH) return false;
    if (p.kh < 1 || p.kw < 1 || p.kh > MAX_TAP || p.kw > MAX_TAP || p.stride < 1) return false;
    if (p.OH < 1 || p.OW < 1 || p.H < 1 || p.W < 1 || p.M != p.NB * p.OH * p.OW) return false;
    if (G > 65535) return false;
    const long HW = (long)p.H * p.W, ohw = (long)p.OH * p.OW;
    const long Wp = (long)(p.OW - 1) * p.stride + p.kw;
    const long SRfull = (long)(p.OH - 1) * p.stride + p.kh;
    // the largest tile whose worst placement stages within the budget: R output rows of I images need R stride + I max(kh - stride, 0) input rows
    int TM = 0;
    long rows_cap = 0;
    for (int tm = 1024; tm >= 128 && !TM; tm /= 2) {
        const long R = std::min<long>((tm - 1) / p.OW + 2, (long)p.NB * p.OH);
        const long I = std::min<long>(p.NB, (R + p.OH - 2) / p.OH + 1);
        const long rows = R * p.stride + I * std::max(p.kh - p.stride, 0);
        if (Ci * rows * Wp <= X_FLOATS && (I + 1) * HW < SPAN_MAX && ohw + tm < SPAN_MAX) { TM = tm; rows_cap = rows; }
    }
    if (!TM) return false;
    const long gx = ((long)p.M + TM - 1) / TM;
    if (gx > 0x7fffffffL) return false;
    const int CO = Co <= 1 ? 1 : (Co <= 2 ? 2 : (Co <= 4 ? 4 : 8));
    DwArgs a;
    a.in = p.in; a.w = p.w; a.w_pos = p.w_pos; a.bias = p.bias; a.bias_pos = p.bias_pos; a.out0 = p.out0; a.out1 = p.out1;
    a.H = p.H; a.W = p.W; a.in_nb = p.in_nb; a.out_nb = p.out_nb; a.kh = p.kh; a.kw = p.kw; a.stride = p.stride; a.pad = p.pad; a.padw = p.pad + p.pad_dw;
    a.OH = p.OH; a.OW = p.OW; a.K = p.K; a.Kp = group_pack_rows(p.K); a.M = p.M; a.relu_in = p.relu_in; a.accumulate = p.accumulate;
    a.out_H = p.out_H; a.out_W = p.out_W; a.out_stride = p.out_stride;
    a.Ci = Ci; a.Co = Co; a.TM = TM; a.Wp = (int)Wp; a.SRfull = (int)SRfull; a.rows_cap = (int)rows_cap;
    a.ws_floats = (p.nhalves * p.K * CO + 3) / 4 * 4;
    a.vec_in = (p.W % 4 == 0 && (reinterpret_cast<uintptr_t>(p.in) & 15) == 0) ? 1 : 0;
    a.r_ohw = 1.f / (float)ohw; a.r_OW = 1.f / (float)p.OW; a.r_HW = 1.f / (float)HW; a.r_W = 1.f / (float)p.W;
    const size_t lds = ((size_t)a.ws_floats + (size_t)Ci * rows_cap * Wp) * sizeof(float);
    const dim3 grid((unsigned)gx, (unsigned)G);
    const int threads = TM / 4;
    const bool vec = p.OW % 4 == 0;
    if (CO == 1) launch_co<1>(a, p.nhalves, vec, grid, threads, lds, s);
    else if (CO == 2) launch_co<2>(a, p.nhalves, vec, grid, threads, lds, s);
    else if (CO == 4) launch_co<4>(a, p.nhalves, vec, grid, threads, lds, s);
    else launch_co<8>(a, p.nhalves, vec, grid, threads, lds, s);
    g_launches++;
    g_last_tile = TM;
    return true;
}
