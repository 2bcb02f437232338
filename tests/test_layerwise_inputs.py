"""CPU checks of tests/layerwise_inputs.py, the truths tests/test_gpu_layerwise_parity.py holds the engine to: the inputs leave (almost) every argmax
decided, every requested layerwise map is well conditioned, and the helper's merge and weight rule are the reference's own lines."""
import numpy as np
import pytest
import torch

import layer_nets as L
import layerwise_inputs as W

NAMES = [c.name for c in L.CASES]
F32, F64 = torch.float32, torch.float64
COUNTS = {}


@pytest.mark.parametrize('name', NAMES + [W.TIE_CASE.name])
def test_clear_rows(name):
    """Both gates, one and three images: at most MAX_UNCLEAR of the (firing, sample) rows are not clear; in every clear row the float32 tape picks the
    float64 tape's element; no max-pool window or MaxFeatureMap pair of the forward is a near-tie."""
    case = W.BY_NAME[name]
    for n in (1, 3):
        assert L.pool_windows_clear(W.tape(case, n, F64)[0]) == [], (name, n)
        for gate in (True, False):
            t64, t32 = W.weights(case, n, gate, F64), W.weights(case, n, gate, F32)
            clear = t64['clear']
            COUNTS[(name, n, gate)] = (int((~clear).sum()), int(clear.size), int((t64['gap'] == 0).sum()))
            assert (~clear).sum() <= W.MAX_UNCLEAR * clear.size, '%s n=%d gate_ge0=%s: %d of %d rows are not clear: change INPUT_SEED[%r]' % (
                name, n, gate, (~clear).sum(), clear.size, name)
            assert np.array_equal(t32['idx'][clear], t64['idx'][clear]), (name, n, gate, np.argwhere(clear & (t32['idx'] != t64['idx'])).tolist())
            assert np.isfinite(t64['w']).all() and np.isfinite(t32['w']).all()


@pytest.mark.parametrize('name', NAMES)
def test_layerwise_maps_are_well_conditioned(name):
    """Every layerwise map the GPU test asks for (three images, every (firing, element slot), four modes; one image, the dense priors) is finite in both
    precisions; where the float64 map is identically zero the float32 map is too; every mode has a non-zero map."""
    case = L.BY_NAME[name]
    for mode in W.MODES:
        nz = z = 0
        for (k, s) in W.sweep_list(case, 3, mode):
            m64, m32 = W.layerwise_map(case, 3, mode, k, s, F64), W.layerwise_map(case, 3, mode, k, s, F32)
            assert bool(torch.isfinite(m64).all()) and bool(torch.isfinite(m32).all()), (name, mode, k, s)
            for b in range(3):
                if float(m64[b].abs().max()) == 0:
                    z += 1
                    assert float(m32[b].abs().max()) == 0, (name, mode, k, s, b)
                else:
                    nz += 1
                    assert float(m32[b].abs().max()) > 0, (name, mode, k, s, b)
        nf = len(W.plain_P(case, 1, mode, F64)) - 1
        for k in range(nf):
            d64, d32 = W.dense_truth(case, mode, k, F64)[1], W.dense_truth(case, mode, k, F32)[1]
            assert bool(torch.isfinite(d64).all()) and bool(torch.isfinite(d32).all()), (name, mode, k)
            assert (float(d64.abs().max()) == 0) == (float(d32.abs().max()) == 0), (name, mode, k)
        COUNTS[(name, mode)] = (nz, z)
        assert nz > 0, (name, mode)


@pytest.mark.parametrize('name', NAMES)
def test_allowances_stay_small(name):
    """What the float32 tape grants the engine stays far below what the GPU test must see (the prior-scaling mutations move a map by 2^-10 ~ 1e-3): the
    tape's own error on every P[k] of the plain sweeps (the capture bound is 4 x that) is at most MAX_PLAIN_E32, and the conditioning allowance of the
    layerwise rows exceeds 1e-4 in at most MAX_COND_SHARE_1E4 of a net's live rows and MAX_COND in none.  A new net or seed that breaks this needs
    another seed, not another bar."""
    case = L.BY_NAME[name]
    conds = []
    for mode in W.MODES:
        for n in (1, 3):
            P32, P64 = W.plain_P(case, n, mode, F32), W.plain_P(case, n, mode, F64)
            for k in range(len(P64) - 1):
                scale = float(P64[k].abs().max())
                e32 = float((P32[k].double() - P64[k]).abs().max()) / max(scale, 1e-300)
                assert e32 <= W.MAX_PLAIN_E32, '%s %s n=%d P[%d]: the float32 tape is off by %.2e: change INPUT_SEED[%r]' % (name, mode, n, k, e32, name)
        elems, _ = W.element_table(case, 3, mode)
        for (k, s) in W.sweep_list(case, 3, mode):
            m64, cond = W.layerwise_map_cond(case, 3, mode, k, s, F64)
            conds += [cond[b] for b in range(3) if elems[k, s, b] >= 0 and float(m64[b].abs().max()) > 0]
    conds = np.array(conds)
    COUNTS[(name, 'cond')] = (float(np.median(conds)), float(np.mean(conds > 1e-4)), float(conds.max()))
    assert conds.max() <= W.MAX_COND and np.mean(conds > 1e-4) <= W.MAX_COND_SHARE_1E4, COUNTS[(name, 'cond')]


def test_calls_hold_an_idle_sweep_and_a_late_image():
    case = L.BY_NAME['projection']
    calls = W.layerwise_calls(case, 3, 'all', 'staggered')
    asc = W.layerwise_calls(case, 3, 'all', 'ascending')
    desc = W.layerwise_calls(case, 3, 'all', 'descending')
    assert len(calls) == len(asc) == len(desc) > 1
    later = 0
    for (F, E, V, src), (Fa, _, _, srca), (Fd, _, _, _) in zip(calls, asc, desc):
        assert 2 <= F.shape[0] <= 5 and F.shape[0] * 3 <= 16
        for G, s_ in ((F, src), (Fa, srca)):
            assert np.all(G[-1] == -1) and s_[-1] == [None] * 3                 # the last sweep is idle for every image ...
            first = [min([int(f) for f in row if f >= 0] or [10 ** 6]) for row in G]
            assert first == sorted(first)                                       # ... and the call ascends: the engine takes the prefix launches
            assert np.any(G[:-1] >= 0)
        assert F[-2, -1] == -1 and src[-2][-1] is None                          # the late image is idle in the last live sweep
        live = F[:-1, -1] >= 0
        assert np.all(F[:-1, -1][live] >= F[:-1, 0][live])                     # the last image starts later
        later += int(np.sum(F[:-1, -1][live] > F[:-1, 0][live]))
        assert np.array_equal(Fa[::-1], Fd) and np.all(Fd[0] == -1)
    assert later > 0
    covered = set(ks for (_, _, _, srca) in asc for row in srca for ks in row if ks is not None)
    assert covered == set(W.sweep_list(case, 3, 'all'))                         # every (firing, element) pair is a row


@pytest.mark.parametrize('count', [1, 3, 8])
@pytest.mark.parametrize('do_max', [False, True])
def test_merge_truth_is_the_reference_merge(count, do_max):
    """merge_truth against oracle/ebp_oracle.py:655-662 written out line by line, on float32 maps: equal bits.  (count 1: the all-zero normalised weights
    and the ones fallback.)"""
    rng = np.random.RandomState(5 + count)
    P_img_valid = [(rng.rand(19, 15) ** 3).astype(np.float32) for _ in range(count)]
    P_subtree_valid = sorted(float(np.float32(v)) for v in rng.rand(count))
    eps = 1e-16
    img = np.float32(P_subtree_valid)
    sn = (img - np.min(img)) / (eps + (np.max(img) - np.min(img)))
    P_subtree_valid_norm = sn if not np.sum(sn) == 0 else np.ones_like(P_subtree_valid)
    stack = np.dstack([float(w) * np.array(P) * (1.0 / (np.max(P) + 1E-12)) for (w, P) in zip(P_subtree_valid_norm, P_img_valid)])
    smap = np.max(stack, axis=2) if do_max else np.sum(stack, axis=2)
    smap /= max(smap.sum(), eps)
    got = W.merge_truth(P_img_valid, P_subtree_valid, do_max)
    assert got.dtype == smap.dtype and np.array_equal(got, smap)
    if count == 1:
        assert np.all(P_subtree_valid_norm == 1)
    got64 = W.merge_truth([p.astype(np.float64) for p in P_img_valid], P_subtree_valid, do_max)
    assert got64.dtype == np.float64 and np.abs(got64 - smap).max() <= 1e-6 * smap.max()


@pytest.mark.parametrize('gate', [True, False])
def test_weight_truth_is_the_reference_rule(gate):
    """weight_truth on one net against oracle/ebp_oracle.py:639-645 written out literally (torch.max / torch.argmax per sample)."""
    case = L.BY_NAME['avg_generic']            # an average pool: exact ties
    x = W.images(case, 3)
    got = W.weight_truth(case, x, gate, F64)
    tape, out = case.tape(x, F64)
    e0, e1 = W.onehot_seeds(case, 3)
    gradlist_mated = tape.true_gradients(out, e0)
    gradlist_nonmated = tape.true_gradients(out, e1)
    n_layers = len(gradlist_mated)
    ties = 0
    for k in range(0, n_layers - 1):
        for b in range(3):
            if gate:
                v = torch.mul(gradlist_mated[k][b] >= 0, -gradlist_nonmated[k][b])
            else:
                v = torch.mul(gradlist_mated[k][b] < 0, -gradlist_nonmated[k][b])
            assert got['w'][k, b] == float(torch.max(v))
            assert v.flatten()[got['idx'][k, b]] == torch.max(v)
            assert got['idx'][k, b] == int(torch.nonzero(v.flatten() == torch.max(v))[0])
            if got['gap'][k, b] != 0:
                assert got['idx'][k, b] == int(torch.argmax(v))
            ties += got['gap'][k, b] == 0
    assert got['w'].shape == (n_layers - 1, 3) and ties > 0


@pytest.mark.parametrize('name', ['projection', 'mfm', 'avg_shortcut_v4', 'encode_tail'])
def test_hook_operands_follow_the_firing_order(name):
    """hook_operands restates the tape's firing order on its own: the names are Tape.backward's, P[k] = a_k relu(g) vanishes wherever a_k does and has its
    shape, and in mode 'all' the gradient a hook passes on is P[k] / (x_k + eps): P[k] = 0 wherever that quotient must be.  one_element_cond is a
    finite, non-negative allowance, and zero for an idle row."""
    case = L.BY_NAME[name]
    ops = W.hook_operands(case, 3, F64)
    t, out = W.tape(case, 3, F64)
    P, names = t.backward(out, W.ebp_seed(case, 3), 'all', 1e-16)
    assert [nm for _, _, nm in ops] == names
    for (a, x, _), p in zip(ops, P):
        assert a.shape == x.shape == p.shape
        assert float(p[a == 0].abs().sum()) == 0
    errs = W.forward_errors(case, 3)
    assert len(errs) == len(ops) and all(0 <= ea < 1e-4 and 0 <= ex < 1e-4 for ea, ex in errs)
    elems, _ = W.element_table(case, 3, 'all')
    for (k, s) in W.sweep_list(case, 3, 'all'):
        _, cond = W.layerwise_map_cond(case, 3, 'all', k, s, F64)
        assert np.isfinite(cond).all() and (cond >= 0).all() and np.all(cond[elems[k, s] < 0] == 0), (name, k, s, cond)


def test_prior_elements():
    P = torch.zeros((3, 2, 2, 3), dtype=F64)
    P[0, 1, 0, 2] = 2.0
    P[0, 0, 1, 1] = 1.0
    P[0, 1, 1, 2] = 0.5
    P[2, 0, 0, 0] = 3.0
    assert W.prior_elements(P) == [[8, 11, 4], [], [0]]
