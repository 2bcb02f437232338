// match.hip -- match calibration on embeddings: row-normalised templates, Euclidean distances of chosen pairs, the k nearest gallery rows of every
// query (net_mate_nonmate_dists.py:118-128, filter_inpaintinggame_for_net.py:105-165, eccv20.py:53-59).  Plain VALU and LDS, no MFMA.
// One distance arithmetic everywhere: the difference of two elements is ONE float32 subtraction (the rounding np.linalg.norm(a - b) makes on float32
// input), its square is exact in float64 (24 x 24 bits), the squares are summed in float64, and sqrt of the sum is rounded to float32 once.  Nothing
// is formed from |a|^2 + |b|^2 - 2 a.b: the decisions downstream compare distances of nearly identical vectors, where that form cancels.
#include "common.h"

namespace {

constexpr int NT = 256;

// ---- K_embed_templates: one workgroup per group ---------------------------------------------------------------------------------------
// tab: offsets [n_groups + 1], then the row list.  Thread t owns elements t, t + 256, ... of the template (D <= 4096: at most 16) and keeps their
// float64 sums in registers; a row's norm is a workgroup reduction in a fixed order, so results do not depend on the launch.
constexpr int TPL_PER = MATCH_MAX_D / NT;

__device__ inline double block_sum_all(double v, double* s_part)
{
    v = wave_sum_all(v);
    __syncthreads();                                       // the previous reduction's readers are done with s_part
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((s_part[0] + s_part[1]) + s_part[2]) + s_part[3];
}

__global__ __launch_bounds__(NT) void embed_templates_kernel(const float* __restrict__ emb, int D, const int* __restrict__ tab, int n_groups,
                                                            int normalize_rows, float* __restrict__ out)
{
    __shared__ double s_part[NT / 64];
    const int g = blockIdx.x;
    const int lo = tab[g], hi = tab[g + 1];
    const int* rows = tab + n_groups + 1;
    double acc[TPL_PER];
#pragma unroll
    for (int j = 0; j < TPL_PER; ++j) acc[j] = 0.0;
    for (int p = lo; p < hi; ++p) {
        const float* e = emb + (size_t)rows[p] * D;
        double v[TPL_PER];
        double ss = 0.0;
#pragma unroll
        for (int j = 0; j < TPL_PER; ++j) {
            const int d = threadIdx.x + j * NT;
            v[j] = d < D ? (double)e[d] : 0.0;
            ss += v[j] * v[j];
        }
        if (normalize_rows) {
            const double nrm = sqrt(block_sum_all(ss, s_part));                          // whitebox.py:778-783
#pragma unroll
            for (int j = 0; j < TPL_PER; ++j) acc[j] += v[j] / nrm;
        } else {
#pragma unroll
            for (int j = 0; j < TPL_PER; ++j) acc[j] += v[j];                            // eccv20.py:53
        }
    }
    double ss = 0.0;
    const double m = normalize_rows ? (double)(hi - lo) : 1.0;                           // the mean of the rows (:108), or their sum
#pragma unroll
    for (int j = 0; j < TPL_PER; ++j) {
        acc[j] /= m;
        ss += acc[j] * acc[j];
    }
    const double nrm = sqrt(block_sum_all(ss, s_part));                                  // :109
#pragma unroll
    for (int j = 0; j < TPL_PER; ++j) {
        const int d = threadIdx.x + j * NT;
        if (d < D) out[(size_t)g * D + d] = (float)(acc[j] / nrm);
    }
}

// ---- K_pair_dists: one wavefront per pair ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void pair_dists_kernel(const float* __restrict__ A, const float* __restrict__ B, int D, const int* __restrict__ pairs,
                                                       int n_pairs, float* __restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const long p = (long)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    if (p >= n_pairs) return;
    const float* a = A + (size_t)pairs[2 * p] * D;
    const float* b = B + (size_t)pairs[2 * p + 1] * D;
    double acc = 0.0;
    for (int d = lane; d < D; d += 64) {
        const float df = a[d] - b[d];
        acc += (double)df * (double)df;
    }
    const double r = sqrt(wave_sum_all(acc));
    if (lane == 0) out[p] = (float)r;
}

// ---- K_nearest_rows: 64 queries per workgroup, the gallery in tiles of 64 rows through LDS ---------------------------------------------
// A thread holds a 4 x 4 block of float64 sums of the 64 x 64 tile; the rows reach it as float4 reads of the two staged tiles, stored d-major
// (row stride NR_LD floats: 16-byte aligned rows, the 16 float4 of a wavefront's gallery read fill one bank row).  After the last D-chunk the tile's
// distances, as float32 bits, replace the staged rows in LDS, and the wavefront that owns a query merges its 64 candidates into the query's sorted
// list of keys (distance bits << 32 | gallery index: the order of the float32 distances, equal ones by index) by rank: a key's place in the merged
// list is the count of keys below it.  A tile none of whose candidates beats the query's k-th best -- nearly all of them, after the first few --
// costs the query one comparison.  The nq x ng matrix never exists.
constexpr int NR_T = 64;                                   // queries per workgroup, gallery rows per tile, and the longest list
constexpr int NR_DC = 32;                                  // elements of D per staged chunk
constexpr int NR_LD = NR_T + 4;
constexpr unsigned long long NR_NONE = ~0ull;
static_assert(NR_T == MATCH_MAX_K, "a list is one wavefront wide");

// rows [r0, r0 + 64) x elements [d0, d0 + 32) of src, zero beyond its n rows and D elements, into dst[d][row]
__device__ inline void stage_rows(const float* __restrict__ src, long n, int D, long r0, int d0, float* dst)
{
    const int d = threadIdx.x & (NR_DC - 1);
#pragma unroll
    for (int pass = 0; pass < NR_T / (NT / NR_DC); ++pass) {
        const int r = pass * (NT / NR_DC) + (threadIdx.x / NR_DC);
        dst[d * NR_LD + r] = (r0 + r < n && d0 + d < D) ? src[(size_t)(r0 + r) * D + d0 + d] : 0.0f;
    }
}

__global__ __launch_bounds__(NT) void nearest_rows_kernel(const float* __restrict__ Q, long nq, const float* __restrict__ G, long ng, int D, int k,
                                                         int exclude_same_index, int* __restrict__ idx, float* __restrict__ dist)
{
    __shared__ __attribute__((aligned(16))) float s_stage[2 * NR_DC * NR_LD];      // the two staged tiles; then the tile's distances, 64 x 64 uint32
    __shared__ unsigned long long s_best[NR_T * NR_T];                             // per query: its list, ascending
    float* s_q = s_stage;
    float* s_g = s_stage + NR_DC * NR_LD;
    unsigned* s_c = reinterpret_cast<unsigned*>(s_stage);
    static_assert(2 * NR_DC * NR_LD >= NR_T * NR_T, "the distances fit where the staged rows were");
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long q0 = (long)blockIdx.x * NR_T;
    for (int i = threadIdx.x; i < NR_T * NR_T; i += NT) s_best[i] = NR_NONE;

    for (long g0 = 0; g0 < ng; g0 += NR_T) {
        double acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
        for (int d0 = 0; d0 < D; d0 += NR_DC) {
            __syncthreads();                               // the previous chunk's readers, or the previous tile's merge (and the lists' initialisation)
            stage_rows(Q, nq, D, q0, d0, s_q);
            stage_rows(G, ng, D, g0, d0, s_g);
            __syncthreads();
#pragma unroll 8
            for (int kk = 0; kk < NR_DC; ++kk) {
                const float4 qv = *reinterpret_cast<const float4*>(s_q + kk * NR_LD + ty * 4);
                const float4 gv = *reinterpret_cast<const float4*>(s_g + kk * NR_LD + tx * 4);
                const float qa[4] = {qv.x, qv.y, qv.z, qv.w}, ga[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float df = qa[i] - ga[j];
                        acc[i][j] += (double)df * (double)df;
                    }
            }
        }
        __syncthreads();                                   // every thread is done with the staged rows
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long q = q0 + ty * 4 + i;
            unsigned bits[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long g = g0 + tx * 4 + j;
                const bool off = g >= ng || (exclude_same_index && g == q);
                bits[j] = off ? 0xFFFFFFFFu : __float_as_uint((float)sqrt(acc[i][j]));
            }
            *reinterpret_cast<uint4*>(s_c + (ty * 4 + i) * NR_T + tx * 4) = make_uint4(bits[0], bits[1], bits[2], bits[3]);
        }
        __syncthreads();
        for (int j = 0; j < NR_T / (NT / 64); ++j) {       // the queries of this wavefront
            const int ql = wave * (NR_T / (NT / 64)) + j;
            if (q0 + ql >= nq) break;
            const unsigned cb = s_c[ql * NR_T + lane];
            const unsigned long long c = cb == 0xFFFFFFFFu ? NR_NONE : ((unsigned long long)cb << 32) | (unsigned long long)(unsigned)(g0 + lane);
            const unsigned long long kth = s_best[ql * NR_T + k - 1];
            if (__ballot(c < kth) == 0ull) continue;
            const unsigned long long b = s_best[ql * NR_T + lane];
            int rc = 0, rb = 0;
            for (int t = 0; t < 64; ++t) {
                const unsigned long long ob = __shfl(b, t), oc = __shfl(c, t);
                rc += (ob < c) + (oc < c);
                rb += (ob < b) + (oc < b);
            }
            // real keys are distinct, so their ranks are; the empty ones share a rank and a value
            if (rb < NR_T) s_best[ql * NR_T + rb] = b;
            if (rc < NR_T) s_best[ql * NR_T + rc] = c;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < NR_T * k; i += NT) {
        const int ql = i / k, l = i - ql * k;
        if (q0 + ql >= nq) break;
        const unsigned long long key = s_best[ql * NR_T + l];
        idx[(size_t)(q0 + ql) * k + l] = (int)(unsigned)(key & 0xFFFFFFFFull);
        dist[(size_t)(q0 + ql) * k + l] = __uint_as_float((unsigned)(key >> 32));
    }
}

}  // namespace

void launch_embed_templates(const float* emb, int D, const int* tab, int n_groups, int normalize_rows, float* out, hipStream_t s)
{
    hipLaunchKernelGGL(embed_templates_kernel, dim3(n_groups), dim3(NT), 0, s, emb, D, tab, n_groups, normalize_rows, out);
}

void launch_pair_dists(const float* A, const float* B, int D, const int* pairs, int n_pairs, float* out, hipStream_t s)
{
    const int per = NT / 64;
    hipLaunchKernelGGL(pair_dists_kernel, dim3((n_pairs + per - 1) / per), dim3(NT), 0, s, A, B, D, pairs, n_pairs, out);
}

void launch_nearest_rows(const float* Q, long nq, const float* G, long ng, int D, int k, int exclude_same_index, int* idx, float* dist, hipStream_t s)
{
    hipLaunchKernelGGL(nearest_rows_kernel, dim3((unsigned)((nq + NR_T - 1) / NR_T)), dim3(NT), 0, s, Q, nq, G, ng, D, k, exclude_same_index, idx, dist);
}
