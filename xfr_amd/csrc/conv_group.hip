// conv_group.hip -- grouped convolutions (Conv2d(groups = G), ResNeXt's 3x3 layers, depthwise layers) as one implicit-GEMM launch over all groups,
// configuration 13.  Activations are channel-major ([C][NB][H][W]), so group g is a dense convolution of the input channels [g Ci, (g + 1) Ci) into
// the output channels [g Co, (g + 1) Co): a GEMM of Co rows, K = Ci kh kw deep, over the M = NB OH OW output pixels.  The backward-data pass is the
// same kernel on the gradient with Ci and Co swapped and the flipped pack (weights.hip), a phase of a strided layer the same with the phase's taps.
//
// Instruction: v_mfma_f32_16x16x4_f32, A = W (lane l: row l & 15, k = l >> 4), B = X (k = l >> 4, column l & 15), D: column l & 15, rows 4 (l >> 4) + r.
// A row block is 16 output channels of ONE group; a group with fewer, or a ragged last block, has zero weight rows in the pack that are computed and
// never stored.  Groups never share a K step: a non-finite activation of one group cannot reach another through 0 x inf (the reference's groups are
// as separate, and its eps = 1e-16 divide makes huge values routine).  The price: Co = 4 pays 4 x, depthwise 16 x the useful matrix-pipe work.
//
// A workgroup (four waves) owns one group, up to RB of its row blocks and 256 columns.  X is staged through LDS in chunks of 32 K rows, one column per
// thread -- coalesced along m; borders, strides, the batch prefix and relu_in resolved there, branch-free.  A thread's 32 loads of a chunk are in flight
// together, and chunk i + 1 is fetched into registers before chunk i is multiplied.  W comes from the per-group pack, staged next to X.  A chunk stages
// and multiplies only its live rows (K = 36: 32 + 4, not 32 + 32).  Every wave takes 64 columns as four interleaved 16-column sub-tiles (sub-tile s =
// columns 4 j + s): one ds_read_b128 gives a lane its X operand of all four (rows 256 floats apart, 16 lanes x 16 bytes a row: no bank conflicts on the
// read groups of MI355X), and after the K loop the four accumulators of a lane hold four neighbouring columns of a row -- one 16-byte store where the
// output is dense.  No atomics: the sums of a launch are the same bits every time.
#include "common.h"

#include <atomic>

namespace {

constexpr int TM = 256;        // columns per workgroup
constexpr int KC = 32;         // K rows per staged chunk
constexpr int THREADS = 256;

typedef float f32x4 __attribute__((ext_vector_type(4)));

std::atomic<long> g_launches{0};

// what the kernel reads of a ConvParams (which carries an epilogue chain a grouped launch never has), and the per-group quantities
struct GroupArgs {
    const float *in, *w, *w_pos, *bias, *bias_pos;
    float *out0, *out1;
    int H, W, in_nb, out_nb, kh, kw, stride, pad, pad_dw, OH, OW, K, M, relu_in, accumulate, out_H, out_W, out_stride;
    int Ci, Co, nrb, chunks, Kp;
};

template <int RB, int NH>
__global__ __launch_bounds__(THREADS) void conv_group_kernel(const GroupArgs p)
{
    const int Ci = p.Ci, Co = p.Co, nrb = p.nrb, chunks = p.chunks, Kp = p.Kp;
    __shared__ __attribute__((aligned(16))) float Xs[KC * TM];
    __shared__ float Ws[NH * RB * KC * GROUP_ROWS];
    const int tid = threadIdx.x;
    const int g = blockIdx.y / chunks;
    const int rb0 = (blockIdx.y % chunks) * RB;
    const int m0 = blockIdx.x * TM;
    const int khw = p.kh * p.kw;
    const int HW = p.H * p.W;
    // this thread's column of the staged tile
    const int m = m0 + tid;
    const bool m_ok = m < p.M;
    int ih0 = 0, iw0 = 0;
    size_t in_base = 0;
    if (m_ok) {
        const int ohw = p.OH * p.OW;
        const int n = m / ohw, r = m - n * ohw;
        const int oh = r / p.OW, ow = r - oh * p.OW;
        ih0 = oh * p.stride - p.pad;
        iw0 = ow * p.stride - (p.pad + p.pad_dw);
        in_base = ((size_t)g * Ci * p.in_nb + n) * HW;
    }
    const int lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, q = lane >> 4;
    f32x4 acc[NH][RB][4];
#pragma unroll
    for (int h = 0; h < NH; ++h)
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
            for (int s = 0; s < 4; ++s) acc[h][rb][s] = f32x4{0.f, 0.f, 0.f, 0.f};
    const bool wave_live = m0 + wave * 64 < p.M;
    // One chunk of X per thread in registers: row k = (ci, a, b), ci-major; zeros for the border, the columns beyond M and the pack's rows beyond K.
    // All of a chunk's loads are in flight together, and chunk i + 1 is fetched before chunk i is multiplied: the MFMAs run under the loads' latency.
    float v[KC];
    const float* src = p.in + in_base;           // this thread's sample in the group's first channel; offsets from here fit 32 bits (tensors stay under 2 GiB)
    const int in_cs = p.in_nb * HW;
    // Branch-free: a lane whose element is padding, beyond K or beyond M reads element 0 of the tensor instead and keeps a zero, so the loads of a chunk
    // issue back to back with no wait between them
    auto load_chunk = [&](int k0) {
        int ci = k0 / khw;
        const int tap = k0 - ci * khw;
        int a = tap / p.kw, b = tap - a * p.kw;
#pragma unroll
        for (int i = 0; i < KC; ++i) {
            const int ih = ih0 + a, iw = iw0 + b;
            const bool ok = m_ok && k0 + i < p.K && (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
            const float x = ok ? src[ci * in_cs + ih * p.W + iw] : p.in[0];
            v[i] = ok ? x : 0.f;
            const bool wb = ++b == p.kw;
            b = wb ? 0 : b;
            a += wb ? 1 : 0;
            const bool wa = a == p.kh;
            a = wa ? 0 : a;
            ci += wa ? 1 : 0;
        }
    };
    load_chunk(0);
    for (int k0 = 0; k0 < p.K; k0 += KC) {
        const int kmax = min(KC, Kp - k0);       // live rows of this chunk, a multiple of 4: nothing beyond them is staged or multiplied
#pragma unroll
        for (int i = 0; i < KC; ++i)
            if (i < kmax) Xs[i * TM + tid] = p.relu_in ? fmaxf(v[i], 0.f) : v[i];
        // stage W: [half][row block][k][16] from the per-group pack (whose rows beyond K are zero)
        for (int i = tid; i < NH * RB * KC * GROUP_ROWS; i += THREADS) {
            const int c = i & (GROUP_ROWS - 1);
            const int kr = (i / GROUP_ROWS) % KC;
            const int rb = (i / (GROUP_ROWS * KC)) % RB;
            const int h = i / (GROUP_ROWS * KC * RB);
            if (kr < kmax && rb0 + rb < nrb) {
                const float* w = h == 0 ? p.w : p.w_pos;
                Ws[i] = w[(((size_t)g * nrb + rb0 + rb) * Kp + k0 + kr) * GROUP_ROWS + c];
            }
        }
        __syncthreads();
        if (k0 + KC < p.K) load_chunk(k0 + KC);
        if (wave_live) {
            for (int ks = 0; ks < kmax / 4; ++ks) {
                const f32x4 xb = *reinterpret_cast<const f32x4*>(&Xs[(4 * ks + q) * TM + wave * 64 + 4 * j]);
#pragma unroll
                for (int h = 0; h < NH; ++h)
#pragma unroll
                    for (int rb = 0; rb < RB; ++rb) {
                        if (rb0 + rb >= nrb) continue;
                        const float wa = Ws[((h * RB + rb) * KC + 4 * ks + q) * GROUP_ROWS + j];
#pragma unroll
                        for (int s = 0; s < 4; ++s) acc[h][rb][s] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa, xb[s], acc[h][rb][s], 0, 0, 0);
                    }
            }
        }
        __syncthreads();
    }
    if (!wave_live) return;
    // the store: lane (j, q) holds rows 4 q + r of every row block at the columns mb .. mb + 3
    const int mb = m0 + wave * 64 + 4 * j;
    if (mb >= p.M) return;
    const int ohw = p.OH * p.OW;
    const size_t out_hw = (size_t)p.out_H * p.out_W;
    const bool dense = p.out_stride == 1 && p.out_H == p.OH && p.out_W == p.OW;
    // 16-byte stores: dense rows whose length keeps every row's start aligned, four live columns
    const bool vec = dense && mb + 3 < p.M && (((size_t)p.out_nb * ohw) & 3) == 0;
    size_t off[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int mm = mb + s;
        if (mm < p.M) {
            const int n = mm / ohw, r = mm - n * ohw;
            const int oh = r / p.OW, ow = r - oh * p.OW;
            off[s] = (size_t)n * out_hw + (size_t)oh * p.out_stride * p.out_W + (size_t)ow * p.out_stride;
        } else off[s] = 0;
    }
#pragma unroll
    for (int h = 0; h < NH; ++h) {
        float* out = h == 0 ? p.out0 : p.out1;
        const float* bias = h == 0 ? p.bias : p.bias_pos;
        const bool vec_h = vec && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
            if (rb0 + rb >= nrb) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int cl = (rb0 + rb) * GROUP_ROWS + 4 * q + r;
                if (cl >= Co) continue;
                const int co = g * Co + cl;
                const float bv = bias ? bias[co] : 0.f;
                float* row = out + (size_t)co * p.out_nb * out_hw;
                if (vec_h) {
                    f32x4 v = {acc[h][rb][0][r] + bv, acc[h][rb][1][r] + bv, acc[h][rb][2][r] + bv, acc[h][rb][3][r] + bv};
                    f32x4* dst = reinterpret_cast<f32x4*>(row + off[0]);
                    if (p.accumulate) { const f32x4 o = *dst; v += o; }
                    *dst = v;
                } else {
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        if (mb + s >= p.M) continue;
                        float v = acc[h][rb][s][r] + bv;
                        if (p.accumulate) v += row[off[s]];
                        row[off[s]] = v;
                    }
                }
            }
        }
    }
}

template <int RB>
void launch_rb(const GroupArgs& a, int nhalves, dim3 grid, hipStream_t s)
{
    if (nhalves == 2) conv_group_kernel<RB, 2><<<grid, THREADS, 0, s>>>(a);
    else conv_group_kernel<RB, 1><<<grid, THREADS, 0, s>>>(a);
}

}  // namespace

long conv_group_launches() { return g_launches.load(); }

bool launch_conv_group(const ConvParams& p, hipStream_t s)
{
    if (!grouped_launch_contract_ok(p)) return false;
    const int G = p.groups, Ci = p.Cin / G, Co = p.CoutTot / G;
    const int nrb = group_row_blocks(Co);
    const int RB = nrb >= 4 ? 4 : (nrb >= 2 ? 2 : 1);
    const int chunks = (nrb + RB - 1) / RB;
    const long gy = (long)G * chunks;
    const long gx = ((long)p.M + TM - 1) / TM;
    if (gy > 65535 || gx > 0x7fffffffL) return false;
    const dim3 grid((unsigned)gx, (unsigned)gy);
    GroupArgs a;
    a.in = p.in; a.w = p.w; a.w_pos = p.w_pos; a.bias = p.bias; a.bias_pos = p.bias_pos; a.out0 = p.out0; a.out1 = p.out1;
    a.H = p.H; a.W = p.W; a.in_nb = p.in_nb; a.out_nb = p.out_nb; a.kh = p.kh; a.kw = p.kw; a.stride = p.stride; a.pad = p.pad; a.pad_dw = p.pad_dw;
    a.OH = p.OH; a.OW = p.OW; a.K = p.K; a.M = p.M; a.relu_in = p.relu_in; a.accumulate = p.accumulate;
    a.out_H = p.out_H; a.out_W = p.out_W; a.out_stride = p.out_stride;
    a.Ci = Ci; a.Co = Co; a.nrb = nrb; a.chunks = chunks; a.Kp = group_pack_rows(p.K);
    if (RB == 4) launch_rb<4>(a, p.nhalves, grid, s);
    else if (RB == 2) launch_rb<2>(a, p.nhalves, grid, s);
    else launch_rb<1>(a, p.nhalves, grid, s);
    g_launches++;
    return true;
}
