"""Device-free truths for the second half of the engine -- layer weights and argmax elements (xfr_subtree_weights), captures
(xfr_ebp_capture), layerwise sweeps with priors (xfr_layerwise_ebp) and the weighted-subtree merge -- on the catalogue of small layer
programs (tests/layer_nets.py), from the oracle tape (oracle/ebp_oracle.py) in float32 and float64.

Inputs: N images `images(case, N)` = case.inputs(N, seed=INPUT_SEED.get(name, 2)), N in {1, 3}; the gate and non-mate seeds are the one-hot rows 0 and 1
of the classify tensor, the EBP seed of the captures and layerwise priors is `ebp_seed(case, N)` (uniform in [0, 1), fixed generator).
Everything is cached per (net, N, ...): tests/test_layerwise_inputs.py (CPU) and tests/test_gpu_layerwise_parity.py share one computation in a session.
"""
import numpy as np
import torch

import layer_nets as L

MODES = ('affineonly', 'affineonly_with_prior', 'all', 'norelu')
# A (firing, sample) row of the weight pass is "clear" -- its argmax element is decided -- when the best and the runner-up value tie exactly in
# float64 (a structural tie, e.g. the input gradient of an average pool: the first index wins) or lie CLEAR_GAP x max|v| apart with both gate
# operands CLEAR_GAP x max|gm| away from the gate's threshold 0.  The float32 tape's error on these gradients is a few 1e-6 relative, so 1e-4 is that
# with room to spare.  A rule for choosing inputs, not a tolerance: at most MAX_UNCLEAR of a net's rows may miss it (test_layerwise_inputs.py).
CLEAR_GAP = 1e-4
MAX_UNCLEAR = 0.05
# input seed per net where the default (2) does not do: stem -- seeds 2 and 3 leave a near-tie max-pool window (pool_windows_clear); bf16x6 -- seed 2
# leaves 2 of 17 rows of the gm < 0 gate with a gate operand 5.8e-5 x max|gm| from zero, and with seed 3 the float32 tape itself is off by 3.5 % of
# max|P[12]| on the plain sweep (one element behind a positive-pass BatchNorm output next to zero; the engine was within 2e-7 there), which would leave the
# capture bound 4 e32 of that firing empty.  MAX_PLAIN_E32 keeps that from coming back unnoticed (test_layerwise_inputs.py).
INPUT_SEED = {'stem': 4, 'bf16x6': 4}
MAX_PLAIN_E32 = 1e-4        # largest float32-tape error on any P[k] of a plain sweep: 4 x this stays under the 2^-10 of the prior-scaling mutations
# the conditioning allowance of the layerwise rows (one_element_cond) must stay small next to what the test is meant to see (2^-10 ~ 1e-3):
# measured per net: median 2e-7 .. 1e-6; share above 1e-4 at most 4.7 % (projection; 4.3 % pool_odd17, 3.3 % halo64, under 3 % elsewhere); maximum 1.5e-3
# (pool_odd17 P[5], 1.1e-3 projection P[1]): the handful of rows above 1e-3 cannot see a 2^-10 change, every other row can
MAX_COND_SHARE_1E4 = 0.05   # at most this share of a net's live rows may have cond > 1e-4 ...
MAX_COND = 2e-3             # ... and none more than this

# One net beyond the catalogue, for the weight pass alone.  subtree_stats_kernel gives a thread every 4096th element of a gradient tensor (16 chunks of
# 256 threads), so its in-thread tie rule only decides between maxima 4096 elements apart: no catalogue net has any (their ties lie inside one
# pooling window, or inside a channel of at most 144 positions).  The input gradient of a global average pool over 65 x 65 = 4225 positions does.
TIE_CASE = L.NetCase('global_4225', (2, 65, 65), L._global_tail(4, 65, False), 'exact ties 4096 elements apart in the weight pass', 31)
BY_NAME = dict(L.BY_NAME, **{TIE_CASE.name: TIE_CASE})

_CACHE = {}


def _cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def images(case, n):
    return case.inputs(n, seed=INPUT_SEED.get(case.name, 2))


def tape(case, n, dtype):
    """(tape, classify tensor id) of images(case, n) in dtype, built once.  Its positive pass -- a function of the recorded forward alone, which
    Tape.backward evaluates anew on every call -- is evaluated once and kept."""
    def run():
        t, out = case.tape(images(case, n), dtype)
        pv = t.positive_pass()
        t.positive_pass = lambda: pv
        return t, out
    return _cached(('tape', case.name, n, dtype), run)


def onehot_seeds(case, n):
    """(e0, e1), each N x D: one-hot rows 0 and 1 of the classify tensor."""
    t, out = tape(case, n, torch.float64)
    d = int(t.T[out].shape[1])
    e0, e1 = torch.zeros((n, d)), torch.zeros((n, d))
    e0[:, 0] = 1.0
    e1[:, 1] = 1.0
    return e0, e1


def ebp_seed(case, n):
    """The seed (N x D, float32) of the plain sweep whose P[k] the captures read and the priors are cut from."""
    t, out = tape(case, n, torch.float64)
    g = torch.Generator().manual_seed(131 * case.seed + 7 * n + 5)
    return torch.rand((n, int(t.T[out].shape[1])), generator=g)


def weight_truth(case, x, gate_ge0, dtype):
    """whitebox.py:684-696 on the tape of the images x: per firing 0 .. nf-1 and sample, w = max v and idx = first argmax of
    v = (gm >= 0 or gm < 0) * (-gn) over the flattened (c, h, w), with gm / gn the true-weight gradients of the one-hot seeds 0 / 1.
    -> dict of [nf, N] arrays: w, idx, gap ((best - runner-up) / scale), scale (max|v|), margin (min |gm| over the two top elements / max|gm|),
    clear (bool), and v: the list of N x (C H W) tensors."""
    t, out = case.tape(x, dtype)
    n, d = int(x.shape[0]), int(t.T[out].shape[1])
    e0, e1 = torch.zeros((n, d)), torch.zeros((n, d))
    e0[:, 0] = 1.0
    e1[:, 1] = 1.0
    gms, gns = t.true_gradients(out, e0), t.true_gradients(out, e1)
    nf = len(gms) - 1
    res = {k: np.zeros((nf, n)) for k in ('w', 'gap', 'scale', 'margin')}
    res['idx'] = np.zeros((nf, n), dtype=np.int64)
    res['v'] = []
    res['shared'] = [k > 0 and gms[k] is gms[k - 1] for k in range(nf)]       # several hooks on one tensor see the same gradient
    for k in range(nf):
        gm, gn = gms[k].flatten(1), gns[k].flatten(1)
        v = ((gm >= 0) if gate_ge0 else (gm < 0)).to(gn.dtype) * (-gn)
        res['v'].append(v)
        for b in range(n):
            if v.shape[1] > 1:
                top, at = torch.topk(v[b], 2)
                best, second = float(top[0]), float(top[1])
            else:
                at, best, second = torch.zeros(2, dtype=torch.long), float(v[b, 0]), float('-inf')
            first = int(torch.nonzero(v[b] == best)[0])
            scale = float(v[b].abs().max())
            others = [int(a) for a in at if int(a) != first][:1]
            res['w'][k, b] = best
            res['idx'][k, b] = first
            res['scale'][k, b] = scale
            res['gap'][k, b] = (best - second) / scale if scale > 0 else 0.0
            res['margin'][k, b] = float(gm[b, [first] + others].abs().min()) / max(float(gm[b].abs().max()), 1e-300)
    res['clear'] = (res['gap'] == 0) | ((res['gap'] > CLEAR_GAP) & (res['margin'] > CLEAR_GAP))
    return res


def weights(case, n, gate_ge0, dtype):
    return _cached(('weights', case.name, n, bool(gate_ge0), dtype), lambda: weight_truth(case, images(case, n), gate_ge0, dtype))


def plain_P(case, n, mode, dtype):
    """Whitebox.P of the plain sweep of images(case, n) seeded with ebp_seed: list of nf + 1 tensors."""
    def run():
        t, out = tape(case, n, dtype)
        return t.backward(out, ebp_seed(case, n), mode, 1e-16)[0]
    return _cached(('P', case.name, n, mode, dtype), run)


def prior_elements(P64_k):
    """Per sample, the flat (c, h, w) indices of up to three elements of P64[k], duplicates dropped: its argmax, its last positive element (the tail
    float4 / the last block of the tensor) and its first positive element.  A sample whose P64[k] is all zero gets []: an idle row."""
    out = []
    for row in P64_k.flatten(1):
        pos = torch.nonzero(row > 0).flatten()
        if pos.numel() == 0:
            out.append([])
            continue
        picks = []
        for e in (int(torch.argmax(row)), int(pos[-1]), int(pos[0])):
            if e not in picks:
                picks.append(e)
        out.append(picks)
    return out


def element_table(case, n, mode):
    """-> (elems [nf, 3, N] int32 with -1 for an idle row, vals [nf, 3, N] float32 = float32(P64[k][elem])) of the plain sweep in `mode`."""
    def run():
        P64 = plain_P(case, n, mode, torch.float64)
        nf = len(P64) - 1
        elems = np.full((nf, 3, n), -1, dtype=np.int32)
        vals = np.zeros((nf, 3, n), dtype=np.float32)
        for k in range(nf):
            flat = P64[k].flatten(1)
            for b, picks in enumerate(prior_elements(P64[k])):
                for s, e in enumerate(picks):
                    elems[k, s, b] = e
                    vals[k, s, b] = np.float32(float(flat[b, e]))
        return elems, vals
    return _cached(('elements', case.name, n, mode), run)


def layerwise_truth(case, x, mode, k, elems, vals, dtype, _tape=None, want_P=False):
    """Whitebox.layerwise_ebp 'elementwise' (whitebox.py:561-581) for the N images x at once: a sweep with a zero seed whose P[k] is replaced by a
    prior that is zero except vals[b] at flat element elems[b] of sample b (elems[b] < 0: an all-zero prior) -> P[-2].sum(1), N x H1 x W1
    (want_P: and the list P).  vals are float32 numbers (the truth's float32 rounding of P64[k][elem], or what the engine captured): the truth does not
    depend on the capture."""
    t, out = _tape if _tape is not None else case.tape(x, dtype)
    seed = torch.zeros((int(x.shape[0]), int(t.T[out].shape[1])))
    shape = tuple(t.true_gradients(out, seed)[int(k)].shape)          # P[k] has the shape of the hooked tensor
    pf = torch.zeros(shape, dtype=dtype).flatten(1)
    for b, (e, v) in enumerate(zip(elems, vals)):
        if int(e) >= 0:
            pf[b, int(e)] = float(np.float32(v))
    P, _ = t.backward(out, seed, mode, 1e-16, priors={int(k): pf.reshape(shape)})
    return (P[-2].sum(1), P) if want_P else P[-2].sum(1)


# ---- conditioning: what a one-element prior does to the rule -----------------------------------------------------------------------------
# A hook returns g = p / (x + eps), elementwise.  With a one-element prior the whole map is a product of a few INDIVIDUAL activations: 1 / x[elem] at
# the prior's hook, then a[el] / x[el] at every later hook the gradient reaches as a single element (through ReLU, BatchNorm, Add ... -- until a
# convolution or a pool spreads it), and a[el] itself where that hook is P[-2].  A float32 forward pass has an ABSOLUTE error E on each tensor, so an
# individual activation v carries the relative error E / v -- 1e-5 and more for the small positive values behind a ReLU, in any float32 implementation,
# the reference's tape included -- and the map's relative error is one draw from that, not a maximum over many elements: the row's e32 is another single
# draw, and says little about the first.  (Measured on the MI355X: the rows outside max(4 e32, FLOOR) are the engine's map times 1 + d, with the
# remainder below 2e-7 and d the relative error of the engine's activation at that element; the engine's absolute error on those tensors is
# 1.0 .. 1.6 times the float32 tape's.)  `cond` states that allowance from the float32 tape's own forward error:
#   cond = sum over those individual activations v of  E32(tensor of v) / v64,   E32(T) = max|T32 - T64|  over the whole tensor,
# (activations that are exactly zero are left out: every implementation divides by eps alone there), and a row passes when
#   e_eng <= max(K_RATIO * e32 + cond, FLOOR).  For a dense prior (every element divides by its own x) cond is the relative
# change of the float64 map when every divisor of the prior's hook moves by E32: the flows behind a hook are non-negative, so that is the worst case.
def hook_operands(case, n, dtype):
    """Per firing, in firing order: (a, x, name) = relu of the true and of the positive-pass value of the hooked call's last input (the operands of
    oracle/ebp_oracle.py:229-231), and the call's class name."""
    def run():
        t, out = tape(case, n, dtype)
        hooks, Pv = t.hooks_by_tensor(), t.positive_pass()
        reach, res = {out}, []
        for k in range(len(t.calls) - 1, -1, -1):
            c = t.calls[k]
            if c.out not in reach:
                continue
            for (kk, _) in hooks.get(c.out, []):
                tin = t.calls[kk].ins[-1]
                res.append((torch.relu(t.T[tin]), torch.relu(Pv[tin]), t.calls[kk].name))
            reach.update(c.ins)
        for (kk, _) in hooks.get(0, []):
            tin = t.calls[kk].ins[-1]
            res.append((torch.relu(t.T[tin]), torch.relu(Pv[tin]), t.calls[kk].name))
        return res
    return _cached(('operands', case.name, n, dtype), run)


def forward_errors(case, n):
    """Per firing: (E32 of a, E32 of x): the float32 tape's largest absolute error on the two operand tensors."""
    def run():
        o64, o32 = hook_operands(case, n, torch.float64), hook_operands(case, n, torch.float32)
        return [(float((a32.double() - a64).abs().max()), float((x32.double() - x64).abs().max())) for (a64, x64, _), (a32, x32, _) in zip(o64, o32)]
    return _cached(('forward_errors', case.name, n), run)


def _divides(mode, name):
    """Does a hook WITHOUT a prior return p / x in this mode?  (oracle/ebp_oracle.py:242-260)"""
    return mode in ('norelu', 'all') or ('Conv' in name) or ('Linear' in name) or ('AvgPool' in name) or ('BatchNorm' in name)


def one_element_cond(case, n, mode, k, elems, P64):
    """cond per sample (see above) of the float64 layerwise sweep whose list of firings is P64 and whose prior sits at flat element elems[b] of P[k]."""
    ops, errs = hook_operands(case, n, torch.float64), forward_errors(case, n)
    nf = len(P64) - 1
    cond = np.zeros(n)
    for b in range(n):
        if int(elems[b]) < 0:
            continue
        a, x, _ = ops[k]
        xv = float(x.flatten(1)[b, int(elems[b])])
        cond[b] += errs[k][1] / xv if xv > 0 else 0.0
        for j in range(k + 1, nf):
            pj = P64[j][b].flatten()
            nz = torch.nonzero(pj).flatten()
            if nz.numel() != 1:
                continue
            el = int(nz[0])
            a, x, name = ops[j]
            av, xv = float(a.flatten(1)[b, el]), float(x.flatten(1)[b, el])
            ratio = _divides(mode, name) and not torch.equal(a, x)        # a == x as tensors: p / x = relu(g) whatever their error
            if ratio or j == nf - 1:
                cond[b] += errs[j][0] / av if av > 0 else 0.0
            if ratio:
                cond[b] += errs[j][1] / xv if xv > 0 else 0.0
    return cond


def layerwise_map(case, n, mode, k, s, dtype):
    """layerwise_truth of element slot s of firing k (element_table) for all N images, cached."""
    return layerwise_map_cond(case, n, mode, k, s, dtype)[0]


def layerwise_map_cond(case, n, mode, k, s, dtype):
    """(layerwise_truth of element slot s of firing k for all N images, cond per sample -- float64 only, else None), cached."""
    def run():
        elems, vals = element_table(case, n, mode)
        m, P = layerwise_truth(case, images(case, n), mode, k, elems[k, s], vals[k, s], dtype, _tape=tape(case, n, dtype), want_P=True)
        return m, (one_element_cond(case, n, mode, k, elems[k, s], P) if dtype == torch.float64 else None)
    return _cached(('map', case.name, n, mode, k, s, dtype), run)


def dense_mask(case, k, shape):
    """A seeded 0 / 1 mask with about half ones, the shape of P[k]."""
    g = torch.Generator().manual_seed(977 * case.seed + k)
    return (torch.rand(shape, generator=g) < 0.5).float()


def dense_truth(case, mode, k, dtype):
    """One image: the sweep with a zero seed whose P[k] is the dense prior float32(P64[k]) * dense_mask -> (prior float32, P[-2].sum(1), cond -- float64
    only, else None)."""
    def run():
        P64 = plain_P(case, 1, mode, torch.float64)
        prior = P64[k].float() * dense_mask(case, k, tuple(P64[k].shape))
        t, out = tape(case, 1, dtype)
        seed = torch.zeros((1, int(t.T[out].shape[1])))
        m = t.backward(out, seed, mode, 1e-16, priors={int(k): prior.to(dtype)})[0][-2].sum(1)
        cond = None
        if dtype == torch.float64 and float(m.abs().max()) > 0:
            x, ex = hook_operands(case, 1, dtype)[k][1], forward_errors(case, 1)[k][1]
            moved = prior.to(dtype) * torch.where(x > ex, x / (x - ex), torch.ones_like(x))           # p / (x - E) = (p x / (x - E)) / x
            m2 = t.backward(out, seed, mode, 1e-16, priors={int(k): moved})[0][-2].sum(1)
            cond = float((m2 - m).abs().max() / m.abs().max())
        return prior, m, cond
    return _cached(('dense', case.name, mode, k, dtype), run)


def merge_truth(maps, w, do_max, eps=1e-16):
    """The reference's merge of the valid subtree maps (whitebox.py:716-726, oracle/ebp_oracle.py:655-662), slots in ascending weight order:
    scale-normalised float32 weights (ones when they sum to zero), w * P / (max P + 1e-12) per map, sum or max over the maps, / max(sum, eps).
    Computed in the precision of the caller's maps (float64 maps: the truth; float32 maps: the reference's own arithmetic)."""
    img = np.float32(w)
    sn = (img - np.min(img)) / (eps + (np.max(img) - np.min(img)))
    norm = sn if not np.sum(sn) == 0 else np.ones_like(img)
    stack = np.dstack([float(wk) * np.array(P) * (1.0 / (np.max(P) + 1E-12)) for (wk, P) in zip(norm, maps)])
    smap = np.max(stack, axis=2) if do_max else np.sum(stack, axis=2)
    smap /= max(smap.sum(), eps)
    return smap


# ---- the rows of the layerwise calls (shared by the GPU test and its child processes) ---------------------------------------------------
def interleaved_calls(case, n, mode):
    """The calls of the three forms, chunk by chunk: descending, ascending, staggered.  The descending call runs whole launches and leaves the gradients of
    its last rows -- the chunk's lowest firing -- in the workspace; the ascending call behind it has its idle sweep in exactly those rows, so a row the
    prefix bookkeeping forgets to zero reads positive values there, not the zeros an earlier idle sweep left.  -> list of (form, call index, call)."""
    forms = [(f, layerwise_calls(case, n, mode, f)) for f in ('descending', 'ascending', 'staggered')]
    return [(f, c, calls[c]) for c in range(len(forms[0][1])) for f, calls in forms]


def sweep_list(case, n, mode):
    """Every (firing, element slot) pair with at least one live image, ascending by firing."""
    elems, _ = element_table(case, n, mode)
    return [(k, s) for k in range(elems.shape[0]) for s in range(3) if (elems[k, s] >= 0).any()]


def layerwise_calls(case, n, mode, form, per_call=5):
    """The calls of one form over sweep_list: a list of (F, E, V, src), each J x N (firing, element, value; firing -1: idle) and src[j][b] = the
    (k, s) whose truth row (j, b) must equal, or None for an idle row.  Every call holds per_call - 1 sweeps of the list and one sweep that is idle
    for EVERY image: in an ascending call no launch of the prefix schedule ever covers its rows, yet its maps must read zero.
    'ascending': the sweeps in ascending firing order, the idle sweep last (the prefix launches and the on-demand zeroing);
    'descending': the same rows, descending, the idle sweep first (whole launches);
    'staggered': ascending, the last image one sweep ahead of the others (its sweeps start later; first[j] is a minimum over images) and idle in the last
    live sweep, then the idle sweep."""
    elems, vals = element_table(case, n, mode)
    sweeps = sweep_list(case, n, mode)
    calls = []
    for c0 in range(0, len(sweeps), per_call - 1):
        chunk = sweeps[c0:c0 + per_call - 1]
        rows = []                                             # per sweep, per image: (k, s) or None
        for j in range(len(chunk)):
            row = []
            for b in range(n):
                jj = j + 1 if (form == 'staggered' and b == n - 1) else j
                ks = chunk[jj] if jj < len(chunk) else None
                row.append(ks if ks is not None and elems[ks[0], ks[1], b] >= 0 else None)
            rows.append(row)
        rows.append([None] * n)
        if form == 'descending':
            rows = rows[::-1]
        J = len(rows)
        F = np.full((J, n), -1, dtype=np.int32)
        E = np.zeros((J, n), dtype=np.int32)
        V = np.zeros((J, n), dtype=np.float32)
        for j in range(J):
            for b in range(n):
                if rows[j][b] is not None:
                    k, s = rows[j][b]
                    F[j, b], E[j, b], V[j, b] = k, elems[k, s, b], vals[k, s, b]
        calls.append((F, E, V, rows))
    return calls
