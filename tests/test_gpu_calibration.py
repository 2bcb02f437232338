"""GPU tests of match calibration: the kernels of match.hip through the C ABI (xfr_embed_templates, xfr_pair_dists, xfr_nearest_rows) and
xfr_amd/calibration.py on the device path.

The yardstick of a template or a distance (calibration_inputs.yardstick): a float64 numpy restatement of the float32 input is the truth; the
reference's own float32 numpy arithmetic is measured against it; every device value must lie within the larger of the reference's largest error and
one float32 ulp of the true value.  The device sums in float64 and rounds once, so it is expected inside half an ulp plus the float32 subtraction it
shares with the reference.  Each test prints both maxima (DESIGN.md section 9e records them).

nearest_rows: indices equal np.argsort of the float32 reference distance matrix, under a condition asserted on the reference alone: in every row the
first k + 1 sorted reference distances differ by at least 8 float32 ulp relative (the reference's float32 sum of D squares is off by a few ulp, so
closer pairs have no defined order).  np.random.RandomState(seed).randn, row-normalised: seed 0 at (257, 257, 128, 8) leaves 27 ulp, seeds 2 / 102 at
(65, 300, 130, 17) 22 ulp, seed 0 at (5, 5, 512, 4) and seeds 0 / 100 at (1, 2, 128, 1) thousands.

End to end the embeddings of both sides come from the same forward calls (the same images in the same chunks), so the yardstick measures the
calibration arithmetic and not the forward."""
import ctypes
import os

import numpy as np
import pytest
import torch

import calibration_inputs as C
import probe_scoring_utils as U
from probe_scoring_utils import mini32      # noqa: F401 (fixture)
from parity_utils import make_images
from xfr_amd import calibration as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng(mini32):
    return mini32._engine(mini32.batch_size)


@pytest.fixture(autouse=True)
def _device_path():
    K.FORCE_HOST = False
    yield
    K.FORCE_HOST = False


def _unit(seed, n, d):
    x = np.random.RandomState(seed).randn(n, d).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _check(what, got, ref32, truth):
    err, ref_err, ok = C.yardstick(got, ref32, truth)
    print('%s: device max error %.3e, float32 reference max error %.3e' % (what, err, ref_err))
    assert np.asarray(got).dtype == np.float32 and np.isfinite(got).all()
    assert ok, what


# ---- embed_templates ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('normalize_rows', [True, False])
@pytest.mark.parametrize('D', [128, 130, 512])
def test_embed_templates(eng, D, normalize_rows):
    rng = np.random.RandomState(D)
    emb = (rng.randn(90, D) * rng.uniform(0.2, 30.0, (90, 1))).astype(np.float32)      # rows of very different norms
    sizes = [1, 2, 5, 64, 1, 5]
    rows = rng.randint(0, 90, sum(sizes))              # arbitrary order, repeats
    rows[3:5] = rows[5]                                # ... also inside a group
    offsets = np.cumsum([0] + sizes)
    got = eng.embed_templates(emb, rows, offsets, normalize_rows=normalize_rows).cpu().numpy()
    assert got.shape == (len(sizes), D)
    _check('embed_templates D=%d normalize_rows=%d' % (D, normalize_rows), got, C.templates_ref(emb, rows, offsets, normalize_rows, np.float32),
           C.templates_ref(emb, rows, offsets, normalize_rows, np.float64))


# ---- pair_dists ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_pairs', [1, 129, 201])
def test_pair_dists(eng, n_pairs):
    D = 130
    a, b = _unit(1, 3, D), _unit(2, 67, D)
    b[5], b[40] = a[1], a[2]                           # identical rows
    b[41] = a[2] * np.float32(1 + 2.0 ** -20)          # and a nearly identical one
    every = np.stack(np.meshgrid(np.arange(3), np.arange(67), indexing='ij'), axis=-1).reshape(-1, 2)
    pairs = every if n_pairs == 201 else every[np.random.RandomState(n_pairs).permutation(201)[:n_pairs]]
    if n_pairs == 1:
        pairs = np.array([[2, 40]])
    got = eng.pair_dists(a, b, pairs).cpu().numpy()
    assert got.shape == (n_pairs,)
    _check('pair_dists %d pairs' % n_pairs, got, C.dists_ref(a, b, pairs, np.float32), C.dists_ref(a, b, pairs, np.float64))
    same = (a[pairs[:, 0]] == b[pairs[:, 1]]).all(axis=1)
    assert same.sum() == {1: 1, 129: same.sum(), 201: 2}[n_pairs]
    assert (got[same] == 0.0).all() and (got[~same] > 0.0).all()


# ---- nearest_rows -------------------------------------------------------------------------------------------------------------------------
def _reference_nearest(Q, G, k, exclude):
    """-> (indices, float32 distances, float64 distances, the smallest relative gap among each row's first k + 1 in float32 ulp)."""
    d32 = np.linalg.norm(Q[:, None, :] - G[None, :, :], axis=2)
    assert d32.dtype == np.float32
    d64 = np.linalg.norm(Q.astype(np.float64)[:, None, :] - G.astype(np.float64)[None, :, :], axis=2)
    if exclude:
        d32[np.arange(len(Q)), np.arange(len(Q))] = np.inf
    order = np.argsort(d32, axis=1, kind='stable')
    s = np.take_along_axis(d32, order, axis=1)[:, :k + 1].astype(np.float64)
    s = s[:, np.isfinite(s).all(axis=0)]
    gap = ((s[:, 1:] - s[:, :-1]) / s[:, 1:]).min() / 2.0 ** -23 if s.shape[1] > 1 else np.inf
    idx = order[:, :k]
    return idx, np.take_along_axis(d32, idx, axis=1), np.take_along_axis(d64, idx, axis=1), gap


@pytest.mark.parametrize('nq,ng,D,k,exclude,seeds', [(1, 2, 128, 1, False, (0, 100)), (257, 257, 128, 8, True, (0, 0)), (65, 300, 130, 17, False, (2, 102)),
                                                     (5, 5, 512, 4, True, (0, 0))])
def test_nearest_rows(eng, nq, ng, D, k, exclude, seeds):
    Q = _unit(seeds[0], nq, D)
    G = Q if seeds[1] == seeds[0] else _unit(seeds[1], ng, D)
    idx, d32, d64, gap = _reference_nearest(Q, G, k, exclude)
    print('nearest_rows (%d, %d, %d, %d): the smallest gap among the first k + 1 reference distances is %.1f ulp' % (nq, ng, D, k, gap))
    assert gap >= 8
    got_idx, got_dist = eng.nearest_rows(Q, G, k, exclude_same_index=exclude)
    got_idx, got_dist = got_idx.cpu().numpy(), got_dist.cpu().numpy()
    assert got_idx.dtype == np.int32 and got_idx.shape == (nq, k) and got_dist.shape == (nq, k)
    assert np.array_equal(got_idx, idx)
    assert (np.diff(got_dist, axis=1) >= 0).all()
    _check('nearest_rows (%d, %d, %d, %d) distances' % (nq, ng, D, k), got_dist, d32, d64)


def test_nearest_rows_orders_equal_distances_by_index(eng):
    G = _unit(3, 140, 128)
    G[70], G[9] = G[3], G[5]                           # equal rows in two tiles of the gallery, and inside one
    G[133] = G[70]
    Q = np.stack([G[3] + np.float32(0.01) * G[20], G[5] + np.float32(0.01) * G[21], G[100]])
    idx, dist = eng.nearest_rows(Q, G, 3)
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    assert idx[0].tolist() == [3, 70, 133] and dist[0, 0] == dist[0, 1] == dist[0, 2]
    assert idx[1].tolist()[:2] == [5, 9] and dist[1, 0] == dist[1, 1]
    assert idx[2, 0] == 100 and dist[2, 0] == 0.0
    idx, _ = eng.nearest_rows(G, G, 2, exclude_same_index=True)
    idx = idx.cpu().numpy()
    assert idx[3].tolist() == [70, 133] and idx[70].tolist() == [3, 133] and idx[133].tolist() == [3, 70] and idx[5, 0] == 9 and idx[9, 0] == 5


# ---- argument errors ----------------------------------------------------------------------------------------------------------------------
def _raw_nearest(eng, q, g, nq, ng, d, k, exclude, idx, dist):
    eng._call(eng.lib.xfr_nearest_rows, q.data_ptr(), nq, g.data_ptr(), ng, d, k, exclude, idx.data_ptr(), dist.data_ptr())


@pytest.mark.parametrize('what,nq,ng,d,k,exclude,text', [('k = 0', 4, 6, 16, 0, 0, 'k = 0'), ('k = 65', 4, 80, 16, 65, 0, 'k = 65'),
                                                         ('k above ng - 1', 6, 6, 16, 6, 1, 'k = 6 of 6'), ('D = 0', 4, 6, 0, 2, 0, 'rows of 0 values'),
                                                         ('D = 4097', 1, 1, 4097, 1, 0, 'rows of 4097 values')])
def test_nearest_rows_refuses(eng, what, nq, ng, d, k, exclude, text):
    q = torch.zeros(8 * 4097, device=eng.device)
    g = torch.zeros(80 * 16 + 4097, device=eng.device)
    idx = torch.full((8 * 65,), -7, device=eng.device, dtype=torch.int32)
    dist = torch.full((8 * 65,), -7.0, device=eng.device)
    with pytest.raises(ValueError, match=text):
        _raw_nearest(eng, q, g, nq, ng, d, k, exclude, idx, dist)
    torch.cuda.synchronize()
    assert (idx == -7).all() and (dist == -7.0).all(), what


def test_row_indices_and_overlaps_are_refused(eng):
    emb = torch.ones((6, 16), device=eng.device)
    out = torch.full((4, 16), -7.0, device=eng.device)
    i32 = lambda v: np.ascontiguousarray(np.asarray(v, dtype=np.int32))
    ptr = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    rows, offsets = i32([0, 6, 1]), i32([0, 2, 3])
    with pytest.raises(ValueError, match='row 6 at place 1'):
        eng._call(eng.lib.xfr_embed_templates, emb.data_ptr(), 6, 16, ptr(rows), ptr(offsets), 2, 1, out.data_ptr())
    rows, offsets = i32([0, 1, 1]), i32([0, 2, 2])
    with pytest.raises(ValueError, match='group 1 is'):
        eng._call(eng.lib.xfr_embed_templates, emb.data_ptr(), 6, 16, ptr(rows), ptr(offsets), 2, 1, out.data_ptr())
    pairs = i32([[0, 0], [5, -1]])
    with pytest.raises(ValueError, match=r'pair 1 is \(5, -1\)'):
        eng._call(eng.lib.xfr_pair_dists, emb.data_ptr(), 6, emb.data_ptr(), 6, 16, ptr(pairs), 2, out.data_ptr())
    pairs = i32([[0, 0], [6, 1]])
    with pytest.raises(ValueError, match=r'pair 1 is \(6, 1\)'):
        eng._call(eng.lib.xfr_pair_dists, emb.data_ptr(), 6, emb.data_ptr(), 6, 16, ptr(pairs), 2, out.data_ptr())
    with pytest.raises(ValueError, match='overlap'):
        eng._call(eng.lib.xfr_pair_dists, emb.data_ptr(), 6, emb.data_ptr(), 6, 16, ptr(i32([[0, 1]])), 1, emb.data_ptr() + 64)
    with pytest.raises(ValueError, match='null argument'):
        eng._call(eng.lib.xfr_pair_dists, emb.data_ptr(), 6, None, 6, 16, ptr(pairs), 2, out.data_ptr())
    torch.cuda.synchronize()
    assert (out == -7.0).all() and (emb == 1.0).all()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def _dists_restated(emb, sizes, dtype):
    """net_mate_nonmate_dists.py:118-128 on raw encodings, in `dtype`."""
    emb = emb.astype(dtype)
    emb = emb / np.linalg.norm(emb, axis=1, keepdims=True)
    mate, nonmate, base = [], [], 0
    for m in sizes:
        e = emb[base:base + 2 + m]
        mate.append(np.linalg.norm(e[0:1] - e[1:2]))
        nonmate.append(np.linalg.norm(e[0:2, np.newaxis, :] - e[np.newaxis, 2:, :], axis=2).reshape(-1))
        base += 2 + m
    return np.stack(mate), np.concatenate(nonmate)


def _batches(n_batches, m, seed):
    x = make_images('stresnet_mini', n_batches * (2 + m), seed=seed)
    for b in range(n_batches):                         # the second mate is its first with a little of a non-mate: a small distance
        x[b * (2 + m) + 1] = 0.9 * x[b * (2 + m)] + 0.1 * x[b * (2 + m) + 2]
    return x, [(x[b * (2 + m):b * (2 + m) + 2], x[b * (2 + m) + 2:(b + 1) * (2 + m)]) for b in range(n_batches)]


def test_mate_nonmate_dists(mini32):
    x, batches = _batches(3, 5, seed=21)
    mate, nonmate = K.mate_nonmate_dists(mini32, batches)
    assert mate.shape == (3,) and nonmate.shape == (3 * 2 * 5,) and mate.dtype == np.float32 and nonmate.dtype == np.float32
    emb = mini32.embeddings(x, norm=False)
    ref32, truth = _dists_restated(emb, [5] * 3, np.float32), _dists_restated(emb, [5] * 3, np.float64)
    _check('mate_nonmate_dists', np.concatenate([mate, nonmate]), np.concatenate(ref32), np.concatenate(truth))
    assert (mate < nonmate.min()).all()


def test_force_host_takes_the_host_path(mini32):
    """One batch, so that both paths see the same forward call.  The host path is the reference's float32 arithmetic on snet.embeddings, to the bit."""
    x, batches = _batches(1, 5, seed=22)
    device = K.mate_nonmate_dists(mini32, batches)
    K.FORCE_HOST = True
    host = K.mate_nonmate_dists(mini32, batches)
    K.FORCE_HOST = False
    emb = mini32.embeddings(x, norm=False)
    ref32, truth = _dists_restated(emb, [5], np.float32), _dists_restated(emb, [5], np.float64)
    assert np.array_equal(host[0], ref32[0]) and np.array_equal(host[1], ref32[1])
    _check('device against host path', np.concatenate(device), np.concatenate(host), np.concatenate(truth))


def _triplet_images(seed):
    x = make_images('stresnet_mini', 14, seed=seed)
    probes, mates, twins, nonmates = x[0:4].clone(), x[4:7].clone(), x[7:11].clone(), x[11:14].clone()
    for i in range(4):                                 # probes near their mates, twins near the non-mates
        probes[i] = 0.5 * probes[i] + 0.5 * mates[i % 3]
        twins[i] = 0.5 * twins[i] + 0.5 * nonmates[i % 3]
    return probes, mates, twins, nonmates


def test_triplet_separability(mini32):
    images = _triplet_images(23)
    K.FORCE_HOST = True
    saved = getattr(mini32, 'match_threshold', None)
    try:
        emb = [mini32.embeddings(im, norm=True).astype(np.float64) for im in images]
        tpl = lambda e: e.mean(axis=0, keepdims=True) / np.linalg.norm(e.mean(axis=0, keepdims=True))
        pr, pg = np.linalg.norm(emb[0] - tpl(emb[1]), axis=1), np.linalg.norm(emb[0] - tpl(emb[3]), axis=1)
        tpr, tpg = np.linalg.norm(emb[2] - tpl(emb[1]), axis=1), np.linalg.norm(emb[2] - tpl(emb[3]), axis=1)
        both = np.sort(np.concatenate([pr, tpr]))      # the threshold: the middle of the widest gap between the distances it is compared with
        widest = np.argmax(np.diff(both))
        mini32.match_threshold = float((both[widest] + both[widest + 1]) / 2)
        thr = mini32.match_threshold
        margins = np.concatenate([np.abs(pr - pg), np.abs(pr - thr), np.abs(tpg - tpr), np.abs(tpr - thr)])
        print('triplet_separability: the smallest reference decision margin is %.3e' % margins.min())
        assert margins.min() > 1e-4
        host = K.triplet_separability(mini32, *images)
        K.FORCE_HOST = False
        device = K.triplet_separability(mini32, *images)
    finally:
        K.FORCE_HOST = False
        if saved is None:
            del mini32.match_threshold
        else:
            mini32.match_threshold = saved
    for h, d in zip(host, device):
        assert h.shape == d.shape == (4, 1) and h.dtype == d.dtype
    assert np.array_equal(host[0], device[0]) and np.array_equal(host[2], device[2])
    assert np.array_equal(host[0][:, 0], (pr < pg) & (pr < thr)) and np.array_equal(host[2][:, 0], (tpg < tpr) & (tpr > thr))
    assert np.abs(host[1] - device[1]).max() < 1e-4 and np.abs(host[3] - device[3]).max() < 1e-4      # below every margin


def test_separability_of_several_masks_in_one_pass(mini32):
    """What separability_table asks per subject: every mask's twins and non-mates behind the probes and mates in one embedding pass.  The host path
    embeds each list in a call of its own, so the two agree to the forward's tolerance across batch compositions, 1e-4 on unit vectors
    (tools/embeddings_sweep.py), not to the yardstick."""
    probes, mates, twins, nonmates = _triplet_images(23)
    masks = [(twins, nonmates), (twins.flip(0), nonmates[:2]), (probes, mates)]
    saved = getattr(mini32, 'match_threshold', None)
    mini32.match_threshold = 0.02
    try:
        device = K._separability(mini32, probes, mates, masks)
        K.FORCE_HOST = True
        host = K._separability(mini32, probes, mates, masks)
    finally:
        K.FORCE_HOST = False
        if saved is None:
            del mini32.match_threshold
        else:
            mini32.match_threshold = saved
    assert len(device) == len(host) == 3
    for d, h in zip(device, host):
        assert np.abs(d[1] - h[1]).max() < 1e-4 and np.abs(d[3] - h[3]).max() < 1e-4
        assert d[1].dtype == np.float32 and d[0].dtype == bool and d[0].shape == (4, 1)
    assert np.abs(host[0][3] - host[1][3]).max() > 2e-4      # the masks differ by more than the tolerance
    assert np.abs(device[2][1]).max() < 1e-4                 # probes as their own twins, mates as non-mates: pg = pr


def test_nearest_nonmates(mini32):
    from scipy.spatial.distance import pdist, squareform
    x = make_images('stresnet_mini', 18, seed=24)
    chunks = [x[2 * i:2 * i + 2] for i in range(9)]
    ids = ['n%06d' % (i * 7) for i in range(9)]
    got = K.nearest_nonmates(mini32, chunks, ids, 3)
    enc = mini32.embeddings(x, norm=False).reshape(9, 2, -1)
    X = np.array([e.sum(axis=0) for e in enc])
    X = X / np.linalg.norm(X, axis=1, keepdims=True)
    d = squareform(pdist(X, metric='euclidean'))
    s = np.sort(d, axis=1)[:, 1:5]
    assert ((s[:, 1:] - s[:, :-1]) / s[:, 1:]).min() >= 8 * 2.0 ** -23
    want = {ids[k]: [ids[j] for j in np.argsort(row)[1:][0:3]] for k, row in enumerate(d)}
    assert got == want
    K.FORCE_HOST = True
    assert K.nearest_nonmates(mini32, chunks, ids, 3) == want


def _write_ijbc_tree(root, n_files=12, n_rows=80):
    import PIL.Image
    import pandas as pd
    os.makedirs(os.path.join(root, 'protocols'))
    os.makedirs(os.path.join(root, 'img'))
    rng = np.random.RandomState(31)
    for f in range(n_files):
        yy, xx = np.mgrid[0:150, 0:170]
        im = np.stack([127 + 120 * np.sin(yy * rng.uniform(0.02, 0.2) + xx * rng.uniform(0.02, 0.2) + rng.uniform(0, 6)) for _ in range(3)], axis=-1)
        PIL.Image.fromarray(im.astype(np.uint8)).save(os.path.join(root, 'img', '%d.png' % f))
    rows = [(1 + r % 5, 'img/%d.png' % rng.randint(n_files), rng.randint(0, 20), rng.randint(0, 20), rng.randint(101, 130), rng.randint(101, 130))
            for r in range(n_rows)]
    pd.DataFrame(rows, columns=['SUBJECT_ID', 'FILENAME', 'FACE_X', 'FACE_Y', 'FACE_WIDTH', 'FACE_HEIGHT']).to_csv(
        os.path.join(root, 'protocols', 'ijbc_metadata.csv'), index=False)


def test_calc_mate_nonmate_dists_drop_in(mini32, tmp_path):
    root = str(tmp_path / 'ijbc')
    _write_ijbc_tree(root)

    class Recorder(object):                            # the host path hands it the frames the draws chose
        def __init__(self):
            self.frames = []

        def embeddings(self, frame, norm=True):
            self.frames.append(frame)
            return _unit(len(self.frames), len(frame), 8)
    rec = Recorder()
    K.calc_mate_nonmate_dists(rec, 2, 5000, str(tmp_path / 'out'), root)
    assert len(rec.frames) == 2 and all(len(f) == 66 for f in rec.frames)
    mate, nonmate = K.calc_mate_nonmate_dists(mini32, 2, 5000, str(tmp_path / 'out'), root)
    assert mate.shape == (2,) and nonmate.shape == (2 * 2 * 64,) and mate.dtype == np.float32 and nonmate.dtype == np.float32
    loaded = [K._network_images(mini32, f) for f in rec.frames]
    want = K.mate_nonmate_dists(mini32, [(im[:2], im[2:]) for im in loaded])
    assert np.array_equal(mate, want[0]) and np.array_equal(nonmate, want[1])
    emb = mini32.embeddings([im for images in loaded for im in images], norm=False)
    ref32, truth = _dists_restated(emb, [64, 64], np.float32), _dists_restated(emb, [64, 64], np.float64)
    _check('calc_mate_nonmate_dists', np.concatenate([mate, nonmate]), np.concatenate(ref32), np.concatenate(truth))
    K.FORCE_HOST = True                                # the host path embeds subject by subject: other chunks, so the forward's tolerance, 1e-4
    host = K.calc_mate_nonmate_dists(mini32, 2, 5000, str(tmp_path / 'out'), root)
    assert host[0].shape == mate.shape and host[1].shape == nonmate.shape and host[0].dtype == np.float32 and host[1].dtype == np.float32
    assert np.abs(host[0] - mate).max() < 1e-4 and np.abs(host[1] - nonmate).max() < 1e-4
