"""What tests/golden/make_golden_calibration.py and the calibration tests share: the stub networks whose embeddings are a seeded function of a file
name (so that the reference's stages run without images or weights), the IJB-C-shaped metadata table, the inpainting-game tree of two subjects,
and the float64 yardstick of the device kernels.  A plain module, no test in it."""
import os
import zlib

import numpy as np

DIM = 64
NET_NAME = 'stubnet'
MATCH_THRESHOLD = 1.0
CALIB_SEED, CALIB_SUBJECTS = 7000, 6      # RANDOM_SEED 7 (* 1000, net_mate_nonmate_dists.py:46): its draw holds the subject with one usable row
METADATA_CSV = 'calibration_ijbc_metadata.csv'


def _randn(tag, scale=1.0):
    return np.random.RandomState(zlib.crc32(tag.encode()) & 0x7FFFFFFF).randn(DIM) * scale


def _unit32(v):
    v = np.asarray(v, dtype=np.float32)
    return v / np.linalg.norm(v, axis=1, keepdims=True)


# ---- calibration distances: IJB-C-shaped metadata -----------------------------------------------------------------------------------------
def metadata_rows():
    """The rows of the metadata table: 14 subjects with 5 to 8 usable rows each, one subject with a single usable row (the len < 2 skip), and
    rows that fail each filter of net_mate_nonmate_dists.py:62-82 (no subject, no box coordinate, a face of at most 100 pixels)."""
    rng = np.random.RandomState(7)
    rows = []
    for s in range(15):
        usable = 1 if s == 9 else 5 + s % 4
        for k in range(usable):
            rows.append((100 + s, 'img/%d_%d.png' % (100 + s, k), rng.randint(0, 50), rng.randint(0, 50), rng.randint(101, 300), rng.randint(101, 300)))
        rows.append((100 + s, 'img/%d_small.png' % (100 + s), 5, 5, 100 - s, 150))                   # Width <= 100
        if s % 3 == 0:
            rows.append((100 + s, 'frames/%d_nobox.png' % (100 + s), np.nan, 7, 200, 200))           # no FACE_X
        if s % 5 == 0:
            rows.append((np.nan, 'img/unknown_%d.png' % s, 3, 3, 200, 200))                          # no subject
    rows.append((109, 'img/109_noheight.png', 4, 4, 180, np.nan))
    return rows


def write_metadata(path):
    import pandas as pd
    pd.DataFrame(metadata_rows(), columns=['SUBJECT_ID', 'FILENAME', 'FACE_X', 'FACE_Y', 'FACE_WIDTH', 'FACE_HEIGHT']).to_csv(path, index=False)


class MetadataNet(object):
    """embeddings(DataFrame, norm=True): a seeded function of FILENAME -- the subject's centre (the number in front of '_') plus the file's own noise."""

    def embeddings(self, frame, norm=True):
        v = np.stack([_randn('subject ' + os.path.basename(fn).split('_')[0]) + _randn(fn, 0.6) for fn in frame['FILENAME']])
        return _unit32(v) if norm else v.astype(np.float32)


# ---- threshold and Platt scaling: synthetic distances -------------------------------------------------------------------------------------
def synthetic_dists(dtype=np.float32):
    rng = np.random.RandomState(11)
    mate = np.abs(rng.normal(0.75, 0.2, 200)).astype(dtype)
    nonmate = np.abs(rng.normal(1.36, 0.09, 12800)).astype(dtype)
    return mate, nonmate


# ---- separability: a two-subject game tree ------------------------------------------------------------------------------------------------
SUBJECTS = {8: (['img/1001.jpg', 'img/1002.jpg', 'frames/1003.png', 'img/1004.jpg'], ['img/1010.jpg', 'img/1011.jpg', 'frames/1012.png']),
            30: (['img/2001.jpg', 'img/2002.jpg', 'img/2003.jpg'], ['img/2010.jpg', 'frames/2011.png'])}      # subject: (probes, references)
MASK_STRENGTH = {0: 1.0, 1: 0.9, 2: 0.1, 3: 0.8, 5: 0.45, 7: 0.55, 6: 0.0, 8: 0.7, 9: 0.3}      # how far a mask's inpainting moves the identity


def write_game_tree(root):
    import pandas as pd
    os.makedirs(root, exist_ok=True)
    for sid, (probes, refs) in SUBJECTS.items():
        rows = [(sid, fn, 'PROBE') for fn in probes] + [(sid, fn, 'REF') for fn in refs]
        pd.DataFrame(rows, columns=['SUBJECT_ID', 'ORIGINAL_FILE', 'TRIPLET_SET']).to_csv(os.path.join(root, 'subj-%d.csv' % sid), index=False)


def game_vector(fn):
    """File name under .../aligned/ -> vector: the subject's centre, moved towards the twin identity by the mask's strength, plus the file's noise."""
    rel = fn.replace(os.sep, '/').split('/aligned/')[-1]
    sid, leaf = rel.split('/')[0], rel.split('/')[-1]
    w = 0.0 if leaf == '00000_truth.png' else MASK_STRENGTH[int(leaf.split('_')[0])]
    return (1.0 - w) * _randn('subject ' + sid) + w * _randn('twin of ' + sid) + _randn(rel, 0.35)


class GameNet(object):
    """embeddings(file names, norm=True) of the game tree; match_threshold as create_wbnet would set it."""
    match_threshold = MATCH_THRESHOLD

    def embeddings(self, fns, norm=True):
        v = np.stack([game_vector(fn) for fn in fns])
        return _unit32(v) if norm else v.astype(np.float32)


def table_arrays(separability):
    """The reference's `separability` DataFrame as plain arrays, rows ordered by (subject, mask, file): what the golden file stores."""
    t = separability.sort_values(['SUBJECT_ID', 'MASK_ID', 'ORIGINAL_FILE'], kind='stable')
    out = {c: np.asarray(t[c].values.tolist()) for c in ('NET', 'SUBJECT_ID', 'ORIGINAL_FILE', 'ORIGINAL_BASENAME', 'TRIPLET_SET', 'MASK_ID', 'OriginalFile',
                                                         'InpaintingFile', 'BestGalleryFile')}
    for c, dt in (('CorrectlyCls', bool), ('TwinCorrectlyCls', bool), ('OrigTripletSim', np.float32), ('TwinTripletSim', np.float32)):
        cells = list(t[c].values)
        assert all(np.shape(v) == (1,) and np.asarray(v).dtype == dt for v in cells), c
        out[c] = np.array([v[0] for v in cells], dtype=dt)
    return out


# ---- the yardstick of the device kernels --------------------------------------------------------------------------------------------------
def ulp32(x):
    """One float32 unit in the last place of |x| (of the smallest normal number below it)."""
    x = np.maximum(np.abs(np.asarray(x, dtype=np.float64)), np.finfo(np.float32).tiny)
    return 2.0 ** (np.floor(np.log2(x)) - 23)


def templates_ref(emb, rows, offsets, normalize_rows, dtype):
    """xfr_embed_templates restated in numpy in `dtype`: float32 is the reference's arithmetic (whitebox.py:778-783, filter_inpaintinggame_for_net.py:
    107-109; eccv20.py:53-54), float64 the truth."""
    emb = np.asarray(emb, dtype=np.float32).astype(dtype)
    out = []
    for g in range(len(offsets) - 1):
        e = emb[np.asarray(rows[offsets[g]:offsets[g + 1]])]
        if normalize_rows:
            e = e / np.linalg.norm(e, axis=1, keepdims=True)
            t = e.mean(axis=0, keepdims=True)
        else:
            t = e.sum(axis=0, keepdims=True)
        out.append(t / np.linalg.norm(t, axis=1, keepdims=True))
    return np.concatenate(out)


def dists_ref(a, b, pairs, dtype):
    a, b, pairs = np.asarray(a, dtype=np.float32).astype(dtype), np.asarray(b, dtype=np.float32).astype(dtype), np.asarray(pairs)
    return np.linalg.norm(a[pairs[:, 0]] - b[pairs[:, 1]], axis=1)


def yardstick(got, ref32, truth):
    """-> (the device's largest error, the float32 reference's largest error, ok).  ok: every device value within the larger of the reference's
    largest error and one float32 ulp of the true value."""
    got, ref32, truth = (np.asarray(v, dtype=np.float64) for v in (got, ref32, truth))
    err, ref_err = np.abs(got - truth), np.abs(ref32 - truth)
    return float(err.max()), float(ref_err.max()), bool(np.all(err <= np.maximum(ref_err.max(), ulp32(truth))))
