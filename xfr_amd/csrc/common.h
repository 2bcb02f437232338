// common.h -- shared declarations of the xfr_amd HIP engine (gfx950 only).
//
// Tensor layout in HBM: every activation / gradient tensor is stored CNHW, i.e. [C][NB][H][W] with NB the
// number of images in flight (N for forward tensors, S*N for the S gradient streams).  With the batch folded
// inside the channel, a 1x1 stride-1 convolution over the whole batch is ONE plain row-major GEMM
// Out[Cout][NB*H*W] = W[Cout][Cin] * In[Cin][NB*H*W], tiles may straddle image boundaries, and the spatial
// index -- the contiguous one -- is the MFMA "B" lane index, so both the im2col gather and the epilogue
// stores are coalesced along it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define XFR_MAX_EW_STEPS 14

// ---- fused elementwise chain (micro-program) -------------------------------------------------------------------------
// Executed per element either by the stand-alone ew_chain kernels or inside the conv_gemm epilogue.
// Index spaces: "g-index" = position in the tensor being produced ([C][SB][HW]); "a-index" = the same (c, hw) in a
// forward-side tensor with B images per channel row (sample b = sb % B).  For forward launches SB == B.
enum {
    EW_HOOK = 0,      // tensor hook (whitebox.py:388-428): a = relu(p0[a]), x = relu(p1[a]) or a; p = a*relu(g); action
    EW_MASK = 1,      // g = p0[a] > 0 ? g : 0                      (in-place ReLU VJP); action 1: the mask is the sign bit of a stored quotient (HOOK_GATE_SIGN)
    EW_SCALE_C = 2,   // g *= p0[c]                                 (BatchNorm VJP with relu(gamma)*invstd)
    EW_SCALE = 3,     // g *= f                                     (Multiply VJP)
    EW_STORE = 4,     // pstore[g] = g.  action 1: no store -- SAVE g (a branch point); action 2: pstore[g] = g, then g = the saved value: the steps
                      // between a save and its store-restore are a side BRANCH of the chain (GEMM epilogues: the main path's hook chain of a
                      // projection-shortcut block next to the shortcut's, resnet50_128.py; one save per chain)
    EW_ADDP = 5,      // g += p0[g]                                 (gradient fan-in / residual add)
    EW_AFFINE_C = 6,  // g = g*p0[c] + p1[c]                        (eval BatchNorm forward)
    EW_RELU = 7,      // g = max(g, 0)
    EW_FORK_POSBN = 8,// pstore[g] = max(g,0)*p0[c] + p1[c]         (positive-pass BatchNorm output, g unchanged)
                      // with p2 != null: ... + (action & 1 ? relu(p2[g]) : p2[g]) -- the positive-pass output of the functional add behind the BatchNorm
                      // (resnet50_128.py torch.add(shortcut, 1, bn)), whose other operand is already there; the BatchNorm's own positive output is then not stored
    EW_MAXHALF_IN = 9,// chain HEAD only (stand-alone kernels): the VJP of torch.max(split[0], split[1]) (lightcnn.py:62).  The chain runs
                      // over the 2*Co-channel Split tensor, the source gradient has Co channels: g = src[c % Co], routed by the true
                      // forward halves a = p0[c % Co], b = p0[c % Co + Co] (ties split evenly like at::maximum); action = Co
    EW_MAXHALF_OUT = 11,// compiled GEMM epilogue only: the same VJP as a FAN-OUT in the epilogue of the GEMM that produces the Co-channel
                      // gradient: for both halves h the routed gradient runs the REST of the chain as channel c + h*Co of the 2*Co-channel
                      // tensor (operands loaded in place at that channel) and is stored there; p0 = true forward halves, action = Co
    EW_ADDP_CO = 13,  // compiled GEMM epilogue only, behind EW_MAXPAIR: g += p0[channel c of the Co-channel tensor] -- the residual add of a Light-CNN
                      // resblock (lightcnn.py:88) on the pair maximum; the even rows then store the SUM
    EW_FORK_POSADD = 14, // ... and, in front of it: pstore[c of Co] = (action & 1 ? relu(g) : g) + (action & 2 ? relu(p0) : p0) -- the Add module's
                      // positive-pass output (its inputs are overridden by A = relu(true input), whitebox.py:315-330); g unchanged
    EW_POOL2_IN = 12, // chain HEAD only (stand-alone kernels): the VJPs of MaxPool2d(2) and AvgPool2d(2) on the SAME input, summed (lightcnn.py:252:
                      // `maxpool(x) + avgpool(x)`).  The chain runs over the pools' input tensor [C][SB][H][W]; the source gradient is the gradient of
                      // the sum, [C][SB][H/2][W/2]: g = 0.25 * src[window] + (argmax[window] == this pixel ? src[window] : 0) -- what AVGPOOL_BWD
                      // followed by an accumulating MAXPOOL_BWD leave in the tensor, bit for bit.  p0 = the max-pool's argmax bytes ([C][B][H/2][W/2],
                      // window-local index dh * 2 + dw), action = W
    EW_AVGUP_IN = 15, // chain HEAD only (stand-alone kernels): the block-input gradient of a down-sampling residual block whose shortcut is
                      // AvgPool2d(2) (+ ConcatChannels) and whose main path starts with a 1x1 / stride 2 convolution (resnet.py:111-149), built in place of
                      // four launches (slice copy, the pooled tensor's hook, the average pool's VJP, the strided GEMM's read-modify-write):
                      //   g(ih, iw) = (0 + hook(src[ih/2, iw/2])) * 0.25  [+ p2[ih/2, iw/2] on the even (ih, iw): the GEMM's result, kept compact]
                      // src = the pooled tensor's gradient ([C][SB][H/2][W/2]: the first C rows of the concatenated gradient); the hook of the pooled
                      // tensor is EW_HOOK's arithmetic on one value (action = HOOK_* or -1 for none, p0 / p1 its a / x at pooled resolution, null p0:
                      // not observed); prior_sb = W.  Same operands, same operations as the four launches: same bits.
                      // action = -2: no pooled source -- the tensor was a zero fill plus strided 1x1 GEMMs (projection shortcut + main path,
                      // resnet50_128.py): g = p2 on the even pixels, 0 elsewhere; the GEMMs accumulate on the compact grid.
    // Lean probe forward (compiled epilogue of a ConvParams::dualacc launch only; g = W accumulator + bias, gp = relu(W) accumulator + bias):
    EW_LEAN_Q = 16,   // FIRST step: q = relu(g) / (relu(gp) + eps) is kept in registers -- the BatchNorm hook's a / (x + eps) (whitebox.py:388-428); g unchanged
    EW_LEAN_XR = 17,  // xr = relu(relu(g) * p0[c] + p1[c] [+ (action & 1 ? relu(p2[g]) : p2[g])]) is kept in registers: what EW_FORK_POSBN would have
                      // stored, clamped -- the x of the ReLU hook behind the BatchNorm [and the functional add]; g unchanged
    EW_LEAN_STORE = 18, // LAST steps.  action 0: pstore[g] = q with its sign bit set where the chain's final value g is <= 0 (the ReLU mask and every
                      // x == a hook of that tensor read the sign, the BatchNorm hook the magnitude); action 1: pstore[g] = g / (xr + eps), the ReLU hook's quotient
    EW_MAXPAIR = 10   // GEMM epilogue only, last step: g = max(g, value of the partner row c ^ 1) -- MaxFeatureMap of a convolution
                      // whose output channels were packed interleaved (row 2c = channel c, row 2c+1 = channel c + Co); the even
                      // rows then store g as channel c of the Co-channel output
};
enum { HOOK_DIV = 0, HOOK_RELU = 1, HOOK_PASS = 2,
       // The "lean" forms of a hook nobody observes (no P store, trace, prior or capture): the probe forward left, instead of the hook's literal
       // operands a and x, what the sweep needs of them (ConvParams::dualacc; plan_fuse.hip lean_rewrite_chain).  Within one ulp per hook of the
       // literal expression for every a a real network produces -- gated by the golden tolerances, not bit for bit.
       HOOK_Q = 3,          // g = relu(g) * |p0[a]|:  p0 holds q = a / (x + eps), computed once in the probe forward (BatchNorm and ReLU hooks)
       HOOK_GATE = 4,       // g = p0[a] > 0 ? relu(g) : 0:  a hook whose x IS its a -- a * relu(g) / (a + eps) = relu(g) wherever a > 1.7e-9, 0 at a = 0
       HOOK_GATE_SIGN = 5   // the same gate read from the SIGN bit of a stored quotient (set where the gated tensor is <= 0)
     };
enum { PRIOR_DIV = 0, PRIOR_PASS = 1, PRIOR_GATEZ = 2 };   // p/(x+eps) | gradient unchanged | (prior>0)*z

struct EwStep {
    int type;
    int action;        // HOOK_*
    const float* p0;
    const float* p1;
    float* pstore;     // HOOK: if non-null, p is stored here (g-index);  STORE / FORK_POSBN: destination
    const float* p2;   // FORK_POSBN: optional addend (g-index), see above
    double* trace;     // HOOK: if non-null, sum(p) per (stream,sample) is accumulated at trace[sb] (stand-alone kernels only)
    float f;           // SCALE: factor
    // HOOK extras for layerwise EBP (whitebox.py:390-392,406-419): at this firing a gradient row sb (stream * B + sample) may
    // have its p OVERRIDDEN by a prior --
    //   prior_elem != null: table over sb; prior_elem[sb] >= 0 means p of row sb is zero except element prior_elem[sb]
    //                       (c*HW+hw within the sample), which is prior_val[sb]   (mode 'elementwise'; many probes x sweeps)
    //   prior_dense != null: row prior_sb gets the dense tensor prior_dense       (mode 'argmax'; one sweep of one image)
    int prior_sb;
    int prior_action;  // PRIOR_* : what the hook returns for such a row
    const int* prior_elem;
    const float* prior_val;
    const float* prior_dense;
    // HOOK: capture p of element cap_elem[sb] (c*HW+hw within the sample; -1: none) of every row sb into cap_dst[sb]
    // (stand-alone kernels only)
    const int* cap_elem;
    float* cap_dst;
    // float4 chain kernel: prefetch slots of p0 / p1 (elementwise.hip, plan_loads); -1: load in place, -2: not needed
    int ls0, ls1;
};

struct EwChain {
    int n;
    EwStep s[XFR_MAX_EW_STEPS];
};

// Operand prefetch plan of a chain.  The per-element operands of all steps -- the forward stashes a / x of the hooks, ReLU
// masks, fan-in gradients -- do not depend on g, and several steps of one chain read the same tensor (in-place ReLU: the
// ReLU hook, the BatchNorm hook and the mask all see the ReLU output).  The float4 chain kernel and the chain epilogue
// of the GEMM issue the distinct loads together before they interpret the steps, instead of one dependent load after
// another.  EwStep::ls0/ls1 hold the slot of p0 / p1.
// Slots 0..2 hold operands indexed like the forward tensors (shared by the gradient streams of one position), slot 3 the one
// gradient-indexed operand (fan-in); slots 5 and 6 are two more forward-indexed ones that only the compiled GEMM epilogues use
// (the 'norelu' / 'all' chains read up to five forward tensors).  4 is not a slot: it encodes "load in place" in a signature.
constexpr int EW_NLOADS = 7;
constexpr int EW_FWD_SLOTS_BASE = 3, EW_FWD_SLOTS_WIDE = 5;
struct EwLoads {
    int nl;                                  // stand-alone kernels: slots 0..nl-1 may be in use (3 may follow a gap)
    const float* lp[EW_NLOADS];
    int lk[EW_NLOADS];                       // 0: indexed like the forward tensors (a-index), 1: like the gradient
};

// Assign prefetch slots.  A load may be hoisted only if nothing in the chain (or the final store to dst) writes the
// buffer it reads: stores land at the same element index in the same thread, after the prefetch.
inline void ew_plan_loads(EwChain& ch, const float* dst, EwLoads& ld, int fwd_slots = EW_FWD_SLOTS_BASE)
{
    static const int fwd_order[EW_FWD_SLOTS_WIDE] = {0, 1, 2, 5, 6};
    ld.nl = 0;
    for (int l = 0; l < EW_NLOADS; ++l) { ld.lp[l] = nullptr; ld.lk[l] = 0; }
    auto written = [&](const float* p) {
        if (p == dst) return true;
        for (int i = 0; i < ch.n; ++i)
            if (ch.s[i].pstore == p) return true;
        return false;
    };
    auto slot_for = [&](const float* p, int kind) -> int {
        if (!p || written(p)) return -1;
        if (kind == 1) {
            if (ld.lp[3] == p) return 3;
            if (ld.lp[3]) return -1;
            ld.lp[3] = p;
            ld.lk[3] = 1;
            return 3;
        }
        for (int i = 0; i < fwd_slots; ++i) {
            const int l = fwd_order[i];
            if (ld.lp[l] == p) return l;
            if (!ld.lp[l]) { ld.lp[l] = p; ld.lk[l] = 0; return l; }
        }
        return -1;
    };
    bool fanned = false;       // behind EW_MAXHALF_OUT the steps run per half at another channel: their operands are loaded in place
    for (int i = 0; i < ch.n; ++i) {
        EwStep& st = ch.s[i];
        st.ls0 = -1;
        st.ls1 = -1;
        if (st.type == EW_MAXHALF_OUT) { fanned = true; continue; }
        if (fanned) {
            if (st.type == EW_HOOK && !st.pstore && !st.trace && (st.action == HOOK_RELU || st.action == HOOK_PASS) && !st.prior_elem && !st.prior_dense && !st.cap_dst) st.ls0 = -2;
            continue;
        }
        if (st.type == EW_HOOK) {
            if (!st.pstore && !st.trace && (st.action == HOOK_RELU || st.action == HOOK_PASS) && !st.prior_elem && !st.prior_dense && !st.cap_dst) { st.ls0 = -2; continue; }
            st.ls0 = slot_for(st.p0, 0);
            if (st.action == HOOK_DIV && st.p1) st.ls1 = slot_for(st.p1, 0);
        } else if (st.type == EW_MASK) {
            st.ls0 = slot_for(st.p0, 0);
        } else if (st.type == EW_ADDP) {
            st.ls0 = slot_for(st.p0, 1);
        }
    }
    ld.nl = ld.lp[3] ? 4 : (ld.lp[2] ? 3 : (ld.lp[1] ? 2 : (ld.lp[0] ? 1 : 0)));   // slots in use form a prefix, except that 3 may follow a gap
}

// Compile-time signature of a planned chain: one 16-bit code per step that does anything.  The GEMM epilogue is
// specialised per signature (conv_gemm.hip: the table chain_sigs.inc lists the signatures the three backbones produce;
// chains outside the table run through the interpreter).  Code = op | s0 << 5 | s1 << 8 | store << 11 | step << 12 with
// s0 / s1 the prefetch slot of p0 / p1 (0..3, 5, 6), 4 = load in place, 7 = none (a hook whose x is its a).
enum { SIG_END = 0, SIG_HOOK_DIV = 1, SIG_HOOK_RELU = 2, SIG_HOOK_PASS = 3, SIG_RELU = 4, SIG_MASK = 5, SIG_SCALE_C = 6, SIG_SCALE = 7,
       SIG_STORE = 8, SIG_ADDP = 9, SIG_AFFINE_C = 10, SIG_FORK_POSBN = 11, SIG_MAXPAIR = 12, SIG_MAXHALF_OUT = 13, SIG_ADDP_CO = 14, SIG_FORK_POSADD = 15,
       SIG_HOOK_Q = 16, SIG_GATE = 17, SIG_GATE_SIGN = 18, SIG_MASK_SIGN = 19, SIG_LEAN_Q = 20, SIG_LEAN_XR = 21, SIG_LEAN_STORE = 22 };
constexpr int sig_op(unsigned c) { return (int)(c & 31u); }
constexpr int sig_s0(unsigned c) { return (int)((c >> 5) & 7u); }
constexpr int sig_s1(unsigned c) { return (int)((c >> 8) & 7u); }
constexpr bool sig_store(unsigned c) { return ((c >> 11) & 1u) != 0; }
constexpr int sig_step(unsigned c) { return (int)((c >> 12) & 15u); }
constexpr bool sig_is_slot(int v) { return v != 4 && v != 7; }

// codes[] of a chain whose prefetch slots are assigned (ew_plan_loads); returns the number of codes, or -1 if the chain
// uses features only the interpreter has (priors, captures, traces)
inline int ew_chain_codes(const EwChain& ch, uint16_t codes[XFR_MAX_EW_STEPS])
{
    int n = 0;
    auto slot = [](int ls) -> unsigned { return ls >= 0 ? (unsigned)ls : 4u; };     // slots 0..3, 5, 6; 4 = in place
    for (int i = 0; i < ch.n; ++i) {
        const EwStep& st = ch.s[i];
        unsigned op = 0, s0 = 7, s1 = 7, store = 0;
        switch (st.type) {
            case EW_HOOK:
                if (st.trace || st.prior_elem || st.prior_dense || st.cap_dst) return -1;
                if (st.ls0 == -2) {                     // p unobserved: relu(g) or the identity
                    if (st.action != HOOK_RELU) continue;
                    op = SIG_RELU;
                    break;
                }
                op = st.action == HOOK_DIV ? SIG_HOOK_DIV : st.action == HOOK_RELU ? SIG_HOOK_RELU : st.action == HOOK_PASS ? SIG_HOOK_PASS
                     : st.action == HOOK_Q ? SIG_HOOK_Q : st.action == HOOK_GATE ? SIG_GATE : SIG_GATE_SIGN;
                s0 = slot(st.ls0);
                if (st.action == HOOK_DIV && st.p1) s1 = slot(st.ls1);
                store = st.pstore ? 1u : 0u;
                break;
            case EW_MASK: op = st.action == 1 ? SIG_MASK_SIGN : SIG_MASK; s0 = slot(st.ls0); break;
            case EW_SCALE_C: op = SIG_SCALE_C; break;
            case EW_SCALE: op = SIG_SCALE; break;
            case EW_STORE: op = SIG_STORE; if (st.action == 1 || st.action == 2) s0 = (unsigned)st.action; break;     // s0: 7 plain, 1 save, 2 store + restore
            case EW_ADDP: op = SIG_ADDP; s0 = slot(st.ls0); break;
            case EW_AFFINE_C: op = SIG_AFFINE_C; break;
            case EW_RELU: op = SIG_RELU; break;
            case EW_FORK_POSBN: op = SIG_FORK_POSBN; if (st.p2) { store = 1; s1 = (unsigned)(st.action & 1); } break;     // store bit: with addend; s1: its clamp flag
            case EW_MAXPAIR: op = SIG_MAXPAIR; break;
            case EW_MAXHALF_OUT: op = SIG_MAXHALF_OUT; break;
            case EW_ADDP_CO: op = SIG_ADDP_CO; break;
            case EW_FORK_POSADD: op = SIG_FORK_POSADD; s0 = (unsigned)(st.action & 3); break;      // the two clamp flags are part of the signature
            case EW_LEAN_Q: op = SIG_LEAN_Q; break;
            case EW_LEAN_XR: op = SIG_LEAN_XR; if (st.p2) { store = 1; s1 = (unsigned)(st.action & 1); } break;     // like SIG_FORK_POSBN
            case EW_LEAN_STORE: op = SIG_LEAN_STORE; s0 = (unsigned)(st.action & 1); break;                          // s0: which quotient
            default: return -1;
        }
        codes[n++] = (uint16_t)(op | (s0 << 5) | (s1 << 8) | (store << 11) | ((unsigned)i << 12));
    }
    return n;
}
// index into the compiled-signature table, -1 if absent (conv_gemm.hip)
int conv_gemm_chain_sig(const EwChain& planned_chain);
int conv_gemm_num_chain_sigs();
void conv_gemm_chain_launch_counts(long* compiled, long* interpreted);
// elementwise.hip: launches per kernel variant of the pools, the normalize pair, the direct stem and the hook-chain kernels (process-wide)
int elementwise_num_variants();
const char* elementwise_variant_name(int i);
long elementwise_variant_launches(int i);

// ---- implicit-GEMM convolution -------------------------------------------------------------------------------
struct ConvParams {
    const float* in;    // [Cin][NB][H][W]
    const float* w;     // packed [K][ldw], K = Cin*kh*kw ordered (ci, kh, kw); column = output channel
    const float* w_pos; // second weight matrix of a dual launch (relu(W)), same packing
    const float* bias;  // [CoutTot] or nullptr
    const float* bias_pos;
    float* out0;        // output of half 0 (w, bias)
    float* out1;        // output of half 1 (w_pos, bias_pos) when nhalves == 2
    int Cin, H, W, NB;  // NB: images covered by this launch (M = NB*OH*OW)
    int in_nb, out_nb;  // images per channel row of the input / output tensors (>= NB: a launch may cover a batch prefix)
    unsigned in_bytes;  // byte size of the input tensor (buffer descriptor range; < 2^31)
    int force_cfg;      // 0 = heuristic tile choice, else a configuration id (tuning / tests)
    int pair_m;         // > 0: the launch covers exactly TWO gradient streams of pair_m = B * OH * OW columns each (M = 2 * pair_m): where pair_m is a
                        // multiple of the tile width the m-tiles are walked stream-interleaved (tile 2j = stream 0's j-th, 2j + 1 = stream 1's j-th),
                        // so the forward-side operands of the epilogue chain -- the same for both streams -- are fetched from HBM once and hit L2 the
                        // second time.  Which workgroup computes which tile changes; no arithmetic does.
    int as_strided;     // a stride-2 1x1 backward-data GEMM whose result stays on its own (compact) grid (EW_AVGUP_IN): tile configuration -- hence K
                        // order -- of the scattering launch it replaces
    // tail balancing (conv_gemm.hip): the last tiles % CUs tiles of a small grid are cut along K into tail_s parts
    // each, so that every CU gets the same share of the final round; parts meet in tail_ws, the last arriver reduces.
    float* tail_ws;     // scratch for the parts' accumulators (nullptr: never balance); one per stream in flight
    unsigned* tail_cnt; // arrival counters, zero between launches (XFR_TAIL_MAX_TILES entries)
    size_t tail_ws_bytes;
    int tail_force;     // 0 = heuristic, 1 = off, S >= 2 = force S parts per tail tile (tuning / tests)
    int tail_q, tail_s; // set by launch_conv_gemm: whole tiles, parts per tail tile (tail_s <= 1: off)
    int tap_major;      // 1: K ordered (kh, kw, ci) instead of (ci, kh, kw); requires Cin % 16 == 0.  2: Cin <= 4 (image stems): K ordered
                        // (kh, kw, 4 channel slots), i.e. K = 4 * kh * kw with zero rows for the missing channels
    int K_logical;      // Cin * kh * kw, for FLOP accounting (== K unless tap_major == 2)
    int kh, kw, stride, pad;
    int pad_dw;         // the columns' padding is pad + pad_dw: a backward-data GEMM of a kernel that is not square (a Linear over an H != W map:
                        // padding kh - 1 on the rows, kw - 1 on the columns); 0 everywhere else
    int OH, OW;
    int K, M;           // M = NB*OH*OW
    int CoutTot, nhalves, ldw;   // CoutTot = output channels per half
    int dualacc;        // 1 (nhalves == 1): every workgroup accumulates W AND relu(W) -- taken from the W fragment in registers, no second pack is read -- over the
                        // same staged input tile; the chain (compiled, first step EW_LEAN_Q) sees both.  The lean probe forward: bias_pos is the second bias
    int relu_in;        // clamp the gathered input at 0 (A = relu(input))
    int bwd;            // 1: a backward-data GEMM of the sweep (bwd_conv_params); 0: a forward convolution
    int split_ok;       // 1: the launch may take the bf16x6 kernel (conv_gemm_split.hip K17) where the layer is one it covers and the grid large enough; 2: whatever the grid (xfr_engine_set_split_gemm)
    int accumulate;     // out += result
    int out_H, out_W, out_stride;  // out_stride > 1: scatter the (OH,OW) grid into an (out_H,out_W) tensor
    int chain_B;        // forward batch for the a-index of the epilogue chain
    float chain_eps;    // eps of the hook divide
    EwChain chain;      // epilogue micro-program applied to half 0 before the final store (n == 0: none)
    EwLoads chain_ld;   // its operand prefetch plan (set by launch_conv_gemm)
    int chain_sig;      // index of the chain's compiled epilogue (chain_sigs.inc), -1: interpreted (set by launch_conv_gemm)
    int chain_interpret; // 1: run the chain through the interpreted epilogue even if a compiled one exists (tests)
    int co_pair;         // Co > 0: MaxFeatureMap convolution whose 2*Co output channels are PACKED interleaved (GEMM row 2c = channel c, row
                         // 2c+1 = channel c + Co): rows are stored at their channel's place, a chain may end in EW_MAXPAIR
    int groups;          // > 1: a grouped convolution (conv_group.hip): group g reads input channels [g Cin / groups, (g + 1) Cin / groups) and writes output
                         // channels [g CoutTot / groups, (g + 1) CoutTot / groups); K = (Cin / groups) * kh * kw is the K of ONE group and w / w_pos are
                         // per-group packs (group_pack_floats below).  0 / 1: an ordinary convolution.  (The field fills the four bytes of padding in front
                         // of `stamps`: no other member moves, and the kernels that take a ConvParams by value are the same instruction for instruction.)
    unsigned long long* stamps;   // tuning hook (xfr_debug_conv_stamps): per wave 8 words -- s_memrealtime at kernel entry, first operands landed,
                                  // K loop done, epilogue entered, exit; HW_ID; XCC_ID; life in shader cycles.  nullptr: off
    int stamps_cap;               // workgroups the stamp buffer holds (later ones do not record)
    int stamp_regions, stamp_seq; // sampled mode (regions > 0): launch `seq` records up to 256 evenly spaced workgroups into region seq % regions
    unsigned long long* span;     // tuning hook (xfr_debug_conv_log): eight words of THIS launch -- block 0's entry time, then exit times of a sample of the workgroups
                                  // (s_memrealtime), i.e. when the launch really started and ended next to the other streams' launches
};
void conv_gemm_set_stamps(unsigned long long* dev_ptr, int capacity_workgroups);
// launch log: every later launch_conv_gemm takes the next eight-word record of log_dev (capacity records) and notes its shape and
// stream on the host; conv_gemm_dump_log writes one CSV line per launch (seq, stream, shape, cfg, start and end in 10 ns ticks)
void conv_gemm_set_log(unsigned long long* log_dev, int capacity);
int conv_gemm_dump_log(const char* path);   // every later launch_conv_gemm records into dev_ptr (nullptr: stop)

constexpr int XFR_TAIL_MAX_TILES = 256;
constexpr size_t XFR_TAIL_WS_BYTES = (size_t)16 << 20;
// false: nothing was launched -- a dual (W / relu(W)) launch carries a chain for which no compiled epilogue exists
bool launch_conv_gemm(const ConvParams& p, hipStream_t s);
// 0 if launch_conv_gemm will accept p's fused chain, else why not (text: conv_gemm_refusal): 1 = dual launch without a compiled epilogue,
// 2 = MaxFeatureMap step (EW_MAXPAIR / EW_MAXHALF_OUT) without a compiled epilogue.  No device work.
int conv_gemm_cannot_launch(const ConvParams& p);
const char* conv_gemm_refusal(int why);
// Configuration ids: which GEMM kernel a launch takes.  The values are public -- ConvParams::force_cfg, XFR_CFG_REMAP, the launch log and profile CSV,
// tools/conv_sweep.py --cfgs, xfr_debug_conv -- and do not change.
enum ConvCfg {
    CFG_K16 = 4,       // 64 x 64 block tile, 16-deep K-steps, three-stage ring
    CFG_K32 = 5,       // ... 32-deep K-steps
    CFG_KS_8_3 = 6,    // intra-workgroup split-K kernel, (BK, ring stages) = (8, 3)
    CFG_KS_4_4 = 7,    // ... (4, 4)
    CFG_BF16X6 = 9,    // the bf16x6 split GEMM (conv_gemm_split.hip)
    CFG_ROW32 = 12,    // 32 x 128 block tile (four waves side by side along m)
    CFG_GROUP = 13,    // the grouped-convolution kernel (conv_group.hip; ConvParams::groups > 1): fp32 MFMA 16x16x4, row blocks of 16 channels of one group
    CFG_DEPTHWISE = 14, // the depthwise kernel (conv_depthwise.hip; a grouped launch with one input or one output channel per group): fp32 on the vector ALU
};
int conv_gemm_pick_cfg(const ConvParams& p);
int conv_gemm_last_cfg();       // the configuration the calling thread's last launch_conv_gemm really ran (CFG_BF16X6: the bf16x6 kernel)
// bf16x6 split GEMM (conv_gemm_split.hip K17, configuration 9; ConvParams::split_ok).  The fp32 pack of a covered layer needs bf16 planes: the engine
// builds them when the weights arrive (conv_gemm_presplit; a pack that has none at a launch gets them there, on that launch's stream, which is then
// drained once).  conv_gemm_forget_split: the packs inside [lo, lo + bytes) changed or go away -- drop their planes.
void conv_gemm_forget_split(const void* lo, size_t bytes);
bool conv_gemm_presplit(const ConvParams& layer, const float* w, hipStream_t s);     // the planes of pack w of that layer (geometry, K, CoutTot, ldw); false: no memory (the pack stays on the fp32 kernels)
int conv_gemm_split_covers(const ConvParams& p);       // a layer xfr_engine_set_split_gemm covers (whatever the launch's grid)
long conv_gemm_split_launches();
// Grouped convolutions (conv_group.hip, configuration 13; ConvParams::groups > 1): one launch over all groups, forward (one or two halves) and
// backward-data alike.  The per-group pack of a layer: for every group, for every row block of 16 output channels of that group, [align_up(K, 4)][16]
// floats -- row k = (ci, kh, kw) ci-major within the group, column = channel within the row block; rows beyond K and columns beyond the group's
// channels are zero.  false: the parameters are not a grouped launch this kernel takes (a chain, dualacc, co_pair), nothing was launched
constexpr int GROUP_ROWS = 16;
inline int group_row_blocks(int co_per_group) { return (co_per_group + GROUP_ROWS - 1) / GROUP_ROWS; }
inline int group_pack_rows(int k_per_group) { return (k_per_group + 3) / 4 * 4; }
inline size_t group_pack_floats(int groups, int co_per_group, int k_per_group)
{
    return (size_t)groups * group_row_blocks(co_per_group) * group_pack_rows(k_per_group) * GROUP_ROWS;
}
inline size_t group_pack_index(int g, int co_local, int k, int co_per_group, int k_per_group)
{
    return (((size_t)g * group_row_blocks(co_per_group) + co_local / GROUP_ROWS) * group_pack_rows(k_per_group) + k) * GROUP_ROWS + co_local % GROUP_ROWS;
}
// What launch_conv_group and launch_conv_depthwise both ask of a launch.  (In a dense output the sample index and pixel of column m are m itself: the
// launch must not cover more pixels than the tensor has.)
inline bool grouped_launch_contract_ok(const ConvParams& p)
{
    const int G = p.groups;
    if (G < 2 || p.Cin % G || p.CoutTot % G || p.chain.n > 0 || p.dualacc || p.co_pair || p.tap_major || p.as_strided || p.pair_m) return false;
    if (p.nhalves < 1 || p.nhalves > 2 || (p.nhalves == 2 && (!p.w_pos || !p.out1)) || !p.w || !p.in || !p.out0 || p.M <= 0) return false;
    if (p.K != p.Cin / G * p.kh * p.kw) return false;
    return p.out_stride >= 1 && (p.OH - 1) * p.out_stride < p.out_H && (p.OW - 1) * p.out_stride < p.out_W && p.NB <= p.in_nb && p.NB <= p.out_nb;
}
bool launch_conv_group(const ConvParams& p, hipStream_t s);
long conv_group_launches();
// Depthwise launches (conv_depthwise.hip, configuration 14): the grouped launches with min(Cin, CoutTot) / groups == 1 -- a depthwise layer's forward
// (any channel multiplier), its backward-data pass, the phases of a strided one -- in fp32 on the vector ALU from one LDS staging of the input.  The
// contract (grouped_launch_contract_ok) and the packs are launch_conv_group's.  false: not a launch this kernel takes (see the caps in its head comment), nothing was launched:
// the caller goes on to launch_conv_group
bool launch_conv_depthwise(const ConvParams& p, hipStream_t s);
long conv_depthwise_launches();
int conv_depthwise_last_tile();   // the tile TM (outputs per workgroup: 1024, 512, 256 or 128) of the calling thread's last launch_conv_depthwise that launched

// g = src[idx]; run chain; dst[idx] = (accumulate ? dst[idx] : 0) + g.   Tensors are [C][SB][HW] for the gradient
// and [C][B][HW] for the forward-side sources (sample b = sb % B).
// SBa <= SB: only the first SBa gradient streams of every channel row are processed (layerwise sweeps whose later
// streams are still identically zero); the float4 kernel honours it, the scalar kernels process all SB.
void launch_ew_chain(const float* src, float* dst, int accumulate, const EwChain& chain,
                     int C, int SB, int B, int HW, float eps, hipStream_t s, int SBa = -1);

// ---- simple forward / backward kernels -----------------------------------------------------------------------
void launch_nchw_to_cnhw(const float* in, float* out, int N, int C, int HW, hipStream_t s);
void launch_cnhw_to_nchw(const float* in, float* out, int N, int C, int HW, hipStream_t s);
// uint8 H x W x C images (as a decoder hands them over) -> the network's fp32 input in CNHW, preprocessing included, in float64 like the
// reference's numpy code: kind 0 = out[c] = (float)(u8[c] - mean[c]) (resnet.py:25-37, whitebox.py:235-258), kind 1 = luminance
// (float)((r/255) w0 + (g/255) w1 + (b/255) w2) into ONE channel (lightcnn.py:19-25 through skimage's rgb2gray)
struct U8Pre { int kind; int channels; double mean[4]; double weight[4]; };
void launch_u8hwc_to_cnhw(const uint8_t* in, float* out, int N, int Cnet, int HW, const U8Pre& pre, hipStream_t s);
// out = maybe_relu( maybe_relu_in(in) * alpha[c] + beta[c] )
void launch_affine_c(const float* in, float* out, const float* alpha, const float* beta, int C, long per_c,
                     int relu_in, int relu_out, hipStream_t s);
void launch_relu(const float* in, float* out, long n, hipStream_t s);
void launch_scale(const float* in, float* out, long n, float f, int relu_in, hipStream_t s);
// out = maybe_relu_out( maybe_relu_in(a) + maybe_relu_in(b) )
void launch_add2(const float* a, const float* b, float* out, long n, int relu_a, int relu_b, int relu_out, hipStream_t s);
// dst (+)= src
void launch_copy_acc(const float* src, float* dst, long n, int accumulate, hipStream_t s);
void launch_maxpool_fwd(const float* in, float* out, uint8_t* idx, int CN, int H, int W, int OH, int OW,
                        int k, int stride, int pad, hipStream_t s);
// out_sum = maxpool2x2(in) + avgpool2x2(in), idx = the max-pool's argmax bytes (may be null), out_pos (may be null) = the positive-pass sum
// (relu_max_pos ? relu(max) : max) + (pos_avg_mode 0: avg, 1: relu(avg), 2: avgpool(relu(in))); bit-identical to the three separate kernels
bool pool2_fwd_ok(const float* in, const uint8_t* idx, int CN, int H, int W, int OH, int OW);
// 5x5 / stride 1 / pad 2 convolution of a one-channel image with MaxFeatureMap, as a direct convolution reading the GEMM's weight pack (rows
// interleaved: 2c = channel c, 2c + 1 = channel c + Co); raw (may be null) [2 Co][NB][H][W], omax [Co][NB][H][W]; bit-identical to the GEMM path
bool stem5_mfm_ok(const float* in, int NB, int H, int W);
// Whitebox.P[-1]: out[n][ci][ih][iw] = relu(img) * relu(conv_backward_data(g, relu(W))) for the first convolution (on demand only)
void launch_image_mwp(const float* g, const float* wp, const float* img, float* out, int Cin, int N, int H, int W, int Cout, int OH, int OW,
                      int kh, int kw, int stride, int pad, int ldw, int kmode, int co_pair, hipStream_t s);
void launch_stem5_mfm(const float* in, const float* wp, int ldw, const float* bias, float* raw, float* omax, int Co, int NB, int H, int W, hipStream_t s);
void launch_pool2_fwd(const float* in, float* out_sum, uint8_t* idx, float* out_pos, int CN, int H, int W, int OH, int OW, int relu_max_pos,
                      int pos_avg_mode, hipStream_t s);
// gin (+)= scatter of gout through the stored argmax; gradient batch SB vs forward batch B
void launch_maxpool_bwd(const float* gout, const uint8_t* idx, float* gin, int accumulate, int C, int SB, int B,
                        int H, int W, int OH, int OW, int k, int stride, int pad, hipStream_t s);
// zero_planes > 0: that many further planes behind the CN pooled ones are written as zeros (the pooled shortcut inside its channel-padded form)
void launch_avgpool_fwd(const float* in, float* out, int CN, int H, int W, int OH, int OW, int k, int stride,
                        int relu_in, hipStream_t s, int zero_planes = 0);
void launch_avgpool_bwd(const float* gout, float* gin, int accumulate, int CN, int H, int W, int OH, int OW,
                        int k, int stride, hipStream_t s);
// out[c] = max(in[c], in[c+Co]) ; optional relu on load
void launch_maxhalves_fwd(const float* in, float* out, int Co, long per_c, int relu_in, hipStream_t s);
// gin[2Co] from gout[Co] using the TRUE forward input tin (ties split evenly, like at::maximum backward)
void launch_maxhalves_bwd(const float* gout, const float* tin, float* gin, int accumulate, int Co, int SB, int B,
                          int HW, hipStream_t s);
// per-sample L2 normalise over channels: tensor [C][NB] (HW == 1)
void launch_normalize_fwd(const float* in, float* out, float* norms, int C, int NB, int relu_in, hipStream_t s);
void launch_normalize_bwd(const float* gout, const float* tin, const float* norms, float* gin, int accumulate,
                          int C, int SB, int B, hipStream_t s);
// seed [S][N][D] (D = C*HW, NCHW order inside a sample) -> gradient tensor [C][S*N][HW]
void launch_seed_to_cnhw(const float* seed, float* g, int SB, int C, int HW, hipStream_t s);
void launch_fill(float* p, long n, float v, hipStream_t s);
// per sample n: v = (gate_ge0 ? gm >= 0 : gm < 0) * (-gn) over the C*HW elements of gm = G[:, n], gn = G[:, N+n] (two gradient streams);
// vmax[n] = max v, vidx[n] = smallest c*HW+hw attaining it   (whitebox.py:689-690)
// weighted-subtree layer weights for all hooked tensors of a sweep in two launches: tensor u = desc[u] ([C][2N][HW]
// gradients, mate stream then non-mate stream); firing f reads tensor f2u[f]; vmax / vidx are [n_firings][N]
struct StatDesc { const float* G; int C; int HW; };
void launch_subtree_stats(const StatDesc* desc_dev, int n_tensors, const int* f2u_dev, int n_firings, float* vmax, int* vidx,
                          void* scratch, int N, int gate_ge0, hipStream_t s);
size_t subtree_stats_scratch_bytes(int N, int n_tensors);

// ---- saliency post-processing --------------------------------------------------------------------------------
// pooled[sb][hw] = sum_c P[c][sb][hw]
void launch_channel_pool(const float* P, float* pooled, int C, int SB, int HW, hipStream_t s);
// sums[sb] = sum over (c,hw) of P[c][sb][hw]  (double accumulation)
void launch_sample_sums(const float* P, double* sums, int C, int SB, int HW, hipStream_t s);
// contrast[n][hw] = sum_c relu(keep * (P[c][n][hw]/sum_n - P[c][N+n][hw]/sum_{N+n})), keep = P/sum >= thr[n] (thr may be null)
void launch_contrast(const float* P, const double* sums, const float* thr, float* out, int C, int N, int HW, hipStream_t s);
// per-sample truncation threshold of whitebox.py:550-553 on m = P[:, n, :]/sum_n: smallest value v such that the
// ascending cumulative sum reaches percentile% of the total at v.
void launch_truncation_threshold(const float* P, const double* sums, float percentile, float* thr, void* scratch,
                                 int C, int N, int HW, hipStream_t s);
size_t truncation_scratch_bytes(int N);
// gaussian(sigma=2, nearest, truncate 4) -> clamp -> /max(sum,eps)    in/out [N][H][W]; tmp same size
void launch_saliency_blur(const float* in, float* tmp, float* out, int N, int H, int W, float eps, hipStream_t s);
// weighted subtree EBP in one call (xfr_weighted_subtree_ebp).  launch_pool_rowmax: launch_channel_pool's sums plus key[sb], the row's max as
// an order-preserving unsigned key (rowmax_from_key turns it back into the float).  launch_gather_rows: dst row pairs[2i+1] = src row pairs[2i].
// launch_reverse_slots: per probe b, slots 0 .. cnt[b]-1 of its topk-slot block in reverse order.  launch_subtree_merge: one workgroup per probe,
// sum (do_max = 0) or max of (wn * P[slot]) * inv over the cnt[b] table entries, then / max(sum, eps) or (mode_u8) the uint8 levels as floats.
struct SubtreeSlot { int slot; float wn; float inv; int pad; };
void launch_pool_rowmax(const float* P, float* pooled, unsigned* key, int C, int SB, int HW, hipStream_t s);
float rowmax_from_key(unsigned key);
void launch_gather_rows(const float* src, float* dst, const int* pairs_dev, int n_pairs, int HW, hipStream_t s);
void launch_reverse_slots(float* store, const int* cnt_dev, int N, int topk, int HW, hipStream_t s);
void launch_subtree_merge(const float* store, const SubtreeSlot* tab_dev, const int* cnt_dev, float* out, int N, int topk, int HW, int do_max,
                          int mode_u8, float eps, hipStream_t s);

// _mwp_to_saliency of ebp_version != 6 (u8_tail.hip): stretch to uint8 levels, Pillow's GaussianBlur(2), stretch again; one workgroup per map of
// H x W <= U8_TAIL_MAX_HW pixels.  Input: float32 maps (in_f), uint8 levels (in_b), or levels held as floats (in_f with levels_as_float); output:
// bytes (out_b) or the levels as floats (out_f, which may be in_f).
constexpr int U8_TAIL_MAX_HW = 65536;
void launch_u8_tail(const float* in_f, const unsigned char* in_b, bool levels_as_float, unsigned char* out_b, float* out_f, int N, int H, int W,
                    float eps, hipStream_t s);

// ---- wavefront (64-lane) shuffle reductions of saliency.hip and strise.hip: the result is complete in lane 0 -------------------
__device__ inline double wave_sum(double v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}

// wave_sum, handed to every lane
__device__ inline double wave_sum_all(double v) { return __shfl(wave_sum(v), 0); }

// One rounded float64 operation each, for the paths of strise.hip and inpaint.hip that are pinned to scipy bit for bit: with contraction switched
// off where the operator stands, no inlining can fuse a product into a sum.  The __dmul_rn / __dadd_rn of the HIP headers are plain operators
// compiled under the translation unit's default, which contracts; the call sites of the two families are not interchangeable.
__device__ inline double mul_rn(double a, double b)
{
#pragma clang fp contract(off)
    return a * b;
}
__device__ inline double add_rn(double a, double b)
{
#pragma clang fp contract(off)
    return a + b;
}
__device__ inline double sub_rn(double a, double b)
{
#pragma clang fp contract(off)
    return a - b;
}
__device__ inline double div_rn(double a, double b)
{
#pragma clang fp contract(off)
    return a / b;
}

// the float64 form of the minimum / maximum reduction of saliency.hip's subtree_merge_kernel
__device__ inline void wave_min_max(double& mn, double& mx)
{
    for (int d = 32; d > 0; d >>= 1) { mn = fmin(mn, __shfl_down(mn, d)); mx = fmax(mx, __shfl_down(mx, d)); }
}

// ---- STRise blackbox saliency (strise.hip; python/xfr/models/blackbox.py:299-442) ----------------------------
// geometry of the sparse masks: images H x W, a grid of gh x gw cells, masks resized to (H + scale) x (W + scale) and cropped at their shift,
// n_elem drawn cells per mask.  cells [n][n_elem] (cell < 0: none -- the all-ones mask), shifts [n][2] = (row shift, column shift).
constexpr int STRISE_MAX_CELLS = 4096;
struct StriseGeom { int H, W, gh, gw, scale, n_elem; double ry, rx; };      // ry = gh / (H + scale), rx = gw / (W + scale)
// out [n][3][H][W] = (float)(mask * u8 + (1 - mask) * fill - mean[c]) in float64; probe uint8 H x W x 3, fill float64 H x W x 3
void launch_strise_masked(const uint8_t* probe, const double* fill, const int* cells, const int* shifts, int n, float* out, const StriseGeom& g,
                          const double* mean, hipStream_t s);
// out [n][H][W]: the float64 masks (parity hook), under the closed-form law or (exact) the exact law of the quantised chain below
void launch_strise_masks(const int* cells, const int* shifts, int n, bool exact, double* out, const StriseGeom& g, hipStream_t s);
// orig [n_refs + n_gal] = similarity of emb0 to every reference / gallery embedding, ginv = 1 / |g| of each
void launch_strise_orig(const float* emb0, const float* refs, int n_refs, const float* gal, int n_gal, int D, double* orig, double* ginv, hipStream_t s);
// scores[i] = contrastive triplet similarity of embedding first + i, i < count
void launch_strise_score(const float* emb, int first, int count, const float* refs, int n_refs, const float* gal, int n_gal, int D, const double* orig,
                         const double* ginv, double* scores, hipStream_t s);
// sal [H][W] = normalised sign * (1 - sum_k w_k mask_k / count); order / group_off: the mask indices grouped by shift (group = sx * scale + sy);
// A [scale^2][gh * gw] and wsum [scale^2] are scratch
void launch_strise_merge(const double* weights, const int* cells, const int* order, const int* group_off, double* A, double* wsum, double count, double sign,
                         double* sal, const StriseGeom& g, hipStream_t s);

// The quantised chain of the generator's black box (whitebox.py:787-806 behind blackbox.py:343): masks by scipy's zoom to the bit, then
// q = uint8((v / 255) * 255).  A row of the image list with a negative shift has no mask: q = probe.
// out [n][3][H][W] = (float)((double)q - mean[c])
void launch_strise_quant(const uint8_t* probe, const double* fill, const int* cells, const int* shifts, int n, float* out, const StriseGeom& g,
                         const double* mean, hipStream_t s);
// out [n][H][W][3] = q (parity hook)
void launch_strise_quant_u8(const uint8_t* probe, const double* fill, const int* cells, const int* shifts, int n, uint8_t* out, const StriseGeom& g,
                            hipStream_t s);
// one output row or column of PIL's 8-bit bilinear resize: pixels [first, first + count) weighted by coef in 2^-22 (xfr_strise_tap)
constexpr int STRISE_MAX_TAPS = 8;
struct StriseTap { int first, count; int coef[STRISE_MAX_TAPS]; };
// one pass of PIL's 8-bit resampling (Resample.c, ImagingResampleHorizontal_8bpc): clip8((2^21 + sum pixel * coef) >> 22), pixels `stride` apart
__device__ inline int resample_u8(const uint8_t* __restrict__ px, int stride, const StriseTap& t)
{
    int acc = 1 << 21;
    for (int i = 0; i < t.count; ++i) acc += (int)px[i * stride] * t.coef[i];
    return min(max(acc >> 22, 0), 255);
}
constexpr int STRISE_LUM_BAND = 16;      // output rows per workgroup of the luminance kernel
constexpr size_t strise_lum_lds_bytes(int rows_max, int W, int in_w) { return (size_t)rows_max * (size_t)(W + in_w) * 3; }
// out [n][1][in_h][in_w] = rgb2gray of the resized and cropped q; row_tab [in_h], col_tab [in_w] on the device; rows_max: the most probe rows one
// band of STRISE_LUM_BAND output rows reads
void launch_strise_quant_lum(const uint8_t* probe, const double* fill, const int* cells, const int* shifts, int n, const StriseTap* row_tab,
                             const StriseTap* col_tab, float* out, const StriseGeom& g, int in_h, int in_w, int rows_max, const double* weight, hipStream_t s);

// ---- inpainting-game scoring (inpaint.hip; python/xfr/inpainting_game/inpainting_game.py:12-197) ----------------------------
// Nested threshold masks are stored as one byte per pixel, first_on: the first level at which the pixel is on, n_levels where it never is; mask l
// is first_on <= l.  A level table travels as a kernel argument: thr[l] is the threshold of level l (non-increasing in l).
constexpr int INPAINT_MAX_LEVELS = 255;
constexpr long INPAINT_MAX_PIXELS = 1L << 24;
struct InpaintLevels { int n; double thr[INPAINT_MAX_LEVELS]; };
constexpr size_t inpaint_scratch_bytes(long n) { return (size_t)n * 32; }      // per map: two key arrays, two index arrays, the running sums
// first_on [n_maps][n] (and cdf [n_maps][n], may be null: the value each pixel is compared by) of float64 maps sal [n_maps][n]; noise [n] or null;
// density != 0: percent-density (the cumulative sum in ascending order, normalised), else s / sum(s) itself.  One workgroup per map.
// total > 0: s = v / total, the caller's sum, instead of the workgroup's own (the launch is then of the maps that share it, usually one)
void launch_inpaint_masks(const double* sal, const double* noise, double max_noise, int include_zero, int density, const InpaintLevels& lv, int n_maps, long n,
                          void* scratch, uint8_t* first_on, double* cdf, hipStream_t s, double total = 0.0);
// out [rows][C][HW]: hybrid first + r of the list (map-major, n_levels per map) = mask ? inpaint : orig; hybrids beyond `total` are the original
void launch_inpaint_blend(const uint8_t* first_on, const float* orig, const float* inpaint, float* out, int C, long HW, long first, int rows, long total,
                          int n_levels, hipStream_t s);
// Soft-edged masks (:68-75): level l of a map is blurred by a separable Gaussian of 2 r + 1 taps, axis 0 then axis 1, edge-clamped, in float64.
// half[j] is the weight at distance j from the centre; soft[l] == 0 leaves level l hard.  Travels as a kernel argument.
constexpr int INPAINT_MAX_BLUR_RADIUS = 64;
struct InpaintBlur { int r; double half[INPAINT_MAX_BLUR_RADIUS + 1]; uint8_t soft[INPAINT_MAX_LEVELS + 1]; };
// out [rows][C][H][W]: hybrid first + r = (float)((1 - m) * orig + m * inpaint) in float64, m the blurred mask; hybrids beyond `total` are the original
void launch_inpaint_soft_blend(const uint8_t* first_on, const float* orig, const float* inpaint, float* out, int C, int H, int W, long first, int rows, long total,
                               int n_levels, const InpaintBlur& blur, hipStream_t s);
// masks [rows][H][W] float64: the blurred masks first .. first + rows of the list
void launch_inpaint_soft_masks(const uint8_t* first_on, double* masks, int H, int W, long first, int rows, int n_levels, const InpaintBlur& blur, hipStream_t s);
// per embedding i < count: pr = |e / |e| - g_orig|, pg = |e / |e| - g_inp| in float64, cls = pg < pr
void launch_inpaint_dist(const float* emb, int count, const float* g_orig, const float* g_inp, int D, double* pg, double* pr, uint8_t* cls, hipStream_t s);
// counts [n_maps][n_levels][3] = |gt & mask|, |gt | mask|, |~gt & mask|
void launch_inpaint_iou(const uint8_t* first_on, const uint8_t* gt, long n, int n_maps, int n_levels, long long* counts, hipStream_t s);

// ---- match calibration (match.hip; net_mate_nonmate_dists.py:118-128, filter_inpaintinggame_for_net.py:105-165, eccv20.py:53-59) ----
constexpr int MATCH_MAX_K = 64;
constexpr int MATCH_MAX_D = 4096;
// out [n_groups][D]: the rows tab[n_groups + 1 + p], p in [tab[g], tab[g + 1]), of emb [.][D], each divided by its norm first when normalize_rows,
// averaged (summed without normalize_rows) and divided by the norm of the result; float64 throughout, one rounding per stored value
void launch_embed_templates(const float* emb, int D, const int* tab, int n_groups, int normalize_rows, float* out, hipStream_t s);
// out [p] = |A[pairs[2 p]] - B[pairs[2 p + 1]]|: float32 differences, their squares summed in float64, one rounding of the root
void launch_pair_dists(const float* A, const float* B, int D, const int* pairs, int n_pairs, float* out, hipStream_t s);
// idx, dist [nq][k]: the k nearest rows of G [ng][D] to every row of Q [nq][D] by that distance, ascending, equal distances by lower index;
// exclude_same_index: query i skips gallery row i.  1 <= k <= MATCH_MAX_K, 1 <= D <= MATCH_MAX_D
void launch_nearest_rows(const float* Q, long nq, const float* G, long ng, int D, int k, int exclude_same_index, int* idx, float* dist, hipStream_t s);

// ---- saliency finishing (finish.hip; python/xfr/show.py:196-222, :131-137, :46-129) ----
constexpr int FINISH_MAX_DIM = 4096;       // the longest axis of a map or of a probe
constexpr int FINISH_MAX_MAPS = 65535;     // maps per call: a grid dimension
constexpr int FINISH_PAD = 12;             // zeros on every side of a map before the spline prefilter
constexpr int FINISH_STATS = 8;            // doubles of per-map statistics
constexpr size_t finish_plane_doubles(int h, int w) { return (size_t)(h + 2 * FINISH_PAD) * (size_t)(w + 2 * FINISH_PAD); }
// stats [n][FINISH_STATS] of float32 maps [n][n_px]: the minimum, the total of the shifted map (totals [n] when given, else the float32 nearest to the
// float64 sum), and what the normalisation and the clip need.  One workgroup per map
void launch_finish_head(const float* maps, int n, long n_px, const float* totals, double* stats, hipStream_t s);
// planes [n][h + 24][w + 24]: the B-spline coefficients of the zero-padded normalised maps (axis 0, then axis 1)
void launch_finish_prefilter(const float* maps, int n, int h, int w, const double* stats, double* planes, hipStream_t s);
// sal [n][H][W], H >= h and W >= w: the 16-tap tensor product at every output pixel, clipped
void launch_finish_resize(const double* planes, int n, int h, int w, int H, int W, const double* stats, double* sal, hipStream_t s);
// sal [n][n_px] = the normalised maps themselves (the probe's size is the map's)
void launch_finish_identity(const float* maps, int n, long n_px, const double* stats, double* sal, hipStream_t s);
// out [n][n_px][3] uint8: the jet overlay of sal on probes [n][n_px][3]; lut [256][3] float64 on the device; writes the maps' ranges into stats
void launch_finish_overlay(const double* sal, const uint8_t* probes, int n, long n_px, double* stats, const double* lut, uint8_t* out, hipStream_t s);

// ---- image intake (intake.hip; python/xfr/models/whitebox.py:787-806 convert_from_numpy, python/xfr/utils.py:39-202) ----
constexpr int INTAKE_MAX_DIM = 4096;       // the longest axis of a crop or of an output
constexpr int INTAKE_MAX_ITEMS = 65535;    // crops per call: a grid dimension
constexpr int INTAKE_MAX_RADIUS = 64;      // the Gaussian pre-filter's radius int(4 sigma + 0.5), sigma = (factor - 1) / 2: factors up to 33.1
constexpr int INTAKE_WEIGHTS = INTAKE_MAX_RADIUS + 1;      // doubles of one kernel: w[0 .. r], w[r] the centre
enum { INTAKE_HEAD_F64 = 0, INTAKE_HEAD_F32 = 1 };
enum { INTAKE_FROM_U8 = 0, INTAKE_FROM_A = 1, INTAKE_FROM_B = 2 };
// one crop of a chunk as the kernels see it.  src: the crop's first byte in the source buffer; ws: its first double in either workspace plane
// (h x w x C doubles each); ry, rx: the radii of the two pre-filter passes, 0 = that axis is skipped; zoom_from: what the zoom reads;
// identity: the output's size is the crop's, no resize; sy, sx = h / H, w / W
struct IntakeItem { long src, ws; int h, w, stride, C, head, ry, rx, zoom_from, identity, pad; double sy, sx; };
// lohi [n][2] = the head of the least and of the largest byte of every crop, all channels
void launch_intake_range(const uint8_t* src, const IntakeItem* items, int n, double* lohi, hipStream_t s);
// the pre-filter passes of a chunk: axis 0 from the bytes into plane A (ry > 0), axis 1 from the bytes into A (ry == 0 < rx), axis 1 from A into B
// (both); wts [n][2][INTAKE_WEIGHTS]; max_elems: the largest h * w * C of the chunk; which: bit p set = some crop takes pass p
void launch_intake_prefilter(const uint8_t* src, const IntakeItem* items, int n, const double* wts, double* plane_a, double* plane_b, long max_elems, int which,
                             hipStream_t s);
// out [n][H][W][3] uint8: zoom, clip, truncate; one channel replicated, a fourth dropped
void launch_intake_zoom(const uint8_t* src, const IntakeItem* items, int n, const double* lohi, const double* plane_a, const double* plane_b, int H, int W,
                        uint8_t* out, hipStream_t s);
// out [n][fh][fw][3] = PIL's 8-bit bilinear resize + crop of q [n][H][W][3] by tap tables on the device (row_tab [fh], col_tab [fw]): the horizontal
// pass into mid [n][H][fw][3], rounded to uint8, then the vertical one
void launch_intake_taps(const uint8_t* q, int n, int H, int W, const StriseTap* row_tab, const StriseTap* col_tab, int fh, int fw, uint8_t* mid, uint8_t* out,
                        hipStream_t s);
