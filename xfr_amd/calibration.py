"""Match calibration of a network and the stages of the reference's evaluation that come before any saliency map, with the reference's names:

    calc_mate_nonmate_dists(net, num_subjects, seed, output_dir, ijbc_path)     python/xfr/inpainting_game/net_mate_nonmate_dists.py:55-144
    match_threshold, platt_scaling, calibrate                                   eval/calculate_net_match_threshold.py:76-99
    triplet_separability, separability_table, include_masks_by_thresholds       eval/filter_inpaintinggame_for_net.py:105-181, :236-250, :261-341
    nearest_nonmates                                                            eval/eccv20.py:47-77
    mate_nonmate_dists                                                          additive: the core of the first, on images already loaded

These are what turns a checkpoint into a usable network object: create_wbnet's match_threshold and platts_scaling belong to the reference's own
weights and are wrong for any other.

Every function that embeds images takes the device path when `net` is an xfr_amd Whitebox: the images are encoded per batch_size chunk, the
encodings stay on the device in one matrix, the templates and distances come from xfr_embed_templates / xfr_pair_dists / xfr_nearest_rows
(include/xfr_amd.h) and only distances and indices cross the bus.  Any other `net` (anything with the reference's embeddings / net.encode), or
FORCE_HOST = True, takes a numpy restatement that is the reference's arithmetic line for line, on what the network's own embeddings() returns.
The device rounds a template or a distance to float32 once, from float64 sums; the reference rounds at every float32 operation, so the two paths
agree to the float32 reference's own error and not to the bit.  nearest_nonmates beyond the kernel's limits (topk > 64,
encodings of more than 4096 values) takes the host restatement too, as the reference does.

match_threshold and platt_scaling stay on the host: a sort, two searchsorted and a 1-D Newton iteration, milliseconds at 128 000 distances.
"""
import glob
import os
import random

import numpy as np

FORCE_HOST = False      # True: every call takes the host restatement (parity tests compare the two paths)

NUM_NONMATES = 64       # net_mate_nonmate_dists.py:93
MASK_IDS = (0, 1, 2, 3, 5, 7, 6, 8, 9)      # filter_inpaintinggame_for_net.py:122
ORIGINAL_PATTERN_REL = 'aligned/{SUBJECT_ID}/{ORIGINAL_BASENAME}/inpainted/00000_truth.png'              # :61-64
INPAINTING_PATTERN_REL = 'aligned/{SUBJECT_ID}/{ORIGINAL_BASENAME}/inpainted/{MASK_ID:05d}_out_0.png'    # :54-56
SEPARABILITY_COLUMNS = ['NET', 'SUBJECT_ID', 'ORIGINAL_FILE', 'ORIGINAL_BASENAME', 'TRIPLET_SET', 'MASK_ID', 'CorrectlyCls', 'OrigTripletSim',
                        'TwinCorrectlyCls', 'TwinTripletSim', 'OriginalFile', 'InpaintingFile', 'BestGalleryFile']      # :236-250


def _is_native(net):
    from .models.whitebox import Whitebox
    return not FORCE_HOST and isinstance(net, Whitebox)


# ---- the device path's two ends ---------------------------------------------------------------------------------------------------------
def _network_images(wb, images, intake='host'):
    """What Whitebox.embeddings makes of its argument (whitebox.py:747-766), one network-format tensor per image -- or, where the device intake
    takes the images (intake 'auto' or 'device'; Whitebox.intake), one uint8 H x W x 3 device tensor per image, the bytes that tensor is made of
    (_device_encodings takes either)."""
    import torch
    from .image_loader import image_loader
    from .models.whitebox import _is_dataframe
    loaded = _is_dataframe(images) or (not isinstance(images, torch.Tensor) and len(images) > 0 and isinstance(images[0], str))
    if loaded:
        u8 = wb._intake_or_none(images, intake)
        if u8 is not None:
            return list(u8)
    if _is_dataframe(images):
        return [wb.convert_from_numpy(im)[0] for im in image_loader(images)]
    if isinstance(images, torch.Tensor):
        return list(images)
    images = list(images)
    if isinstance(images[0], torch.Tensor):
        return images
    if isinstance(images[0], np.ndarray) and images[0].shape[0] in (1, 3):
        return [torch.from_numpy(np.ascontiguousarray(im)).float() for im in images]
    return [wb.convert_from_numpy(im)[0] for im in image_loader(images)]


def _device_encodings(wb, images):
    """The raw encodings of an iterable of network-format images as one n x D device matrix, encoded in chunks of wb.batch_size in the order given
    (the chunks Whitebox.embeddings makes of the same list)."""
    import torch
    eng, mark = wb._engine(wb.batch_size), wb.net._mark('encode')
    out, chunk = [], []

    def is_u8(im):
        return isinstance(im, torch.Tensor) and im.dtype == torch.uint8

    def flush():
        if is_u8(chunk[0]):                  # the device intake's bytes: the engine's own pixel arithmetic in front of the same forward
            out.append(eng.forward_u8(torch.stack(chunk), mark).reshape(len(chunk), -1))
        else:
            x = torch.stack([torch.as_tensor(im, dtype=torch.float32) for im in chunk])
            out.append(eng.forward(x, mark).reshape(len(chunk), -1))
        del chunk[:]
    for im in images:
        if chunk and is_u8(im) != is_u8(chunk[0]):      # a list that mixes the two kinds: no chunk does
            flush()
        chunk.append(im)
        if len(chunk) == wb.batch_size:
            flush()
    if chunk:
        flush()
    return eng, torch.cat(out, dim=0)


# ---- mate and non-mate distances --------------------------------------------------------------------------------------------------------
def _host_dists(embeddings):
    """net_mate_nonmate_dists.py:123-128 for the embeddings of one subject's (two mates, m non-mates): -> (scalar, 2 x m)."""
    mate_embeds = embeddings[0:2]
    mate_embeds = mate_embeds[:, np.newaxis, :]
    nonmate_embeds = embeddings[np.newaxis, 2:, :]
    return np.linalg.norm(mate_embeds[0] - mate_embeds[1]), np.linalg.norm(mate_embeds - nonmate_embeds, axis=2)


def _stack_dists(mate_dists, nonmate_dists):
    """:141-142."""
    return np.stack(mate_dists), np.stack(nonmate_dists).reshape((-1,))


def mate_nonmate_dists(net, batches):
    """Additive: the core of calc_mate_nonmate_dists on loaded images.  batches: an iterable of (two mate images, m non-mate images), every image in
    network format.  -> (mate_dists float32 [S], nonmate_dists float32 [sum of 2 m]).  On the device all batches go through one embedding pass, one
    xfr_embed_templates call for the row normalisation and one xfr_pair_dists call."""
    if not _is_native(net):
        mate_dists, nonmate_dists = [], []
        for mates, nonmates in batches:
            d_mate, d_non = _host_dists(net.embeddings(list(mates) + list(nonmates), norm=True))
            mate_dists.append(d_mate)
            nonmate_dists.append(d_non.reshape(-1))
        return np.stack(mate_dists), np.concatenate(nonmate_dists)
    sizes = []

    def images():
        for mates, nonmates in batches:
            mates, nonmates = list(mates), list(nonmates)
            if len(mates) != 2 or not nonmates:
                raise ValueError('a batch is (two mate images, at least one non-mate image), got %d and %d' % (len(mates), len(nonmates)))
            sizes.append(len(nonmates))
            for im in mates + nonmates:
                yield im
    eng, enc = _device_encodings(net, images())
    n = enc.shape[0]
    unit = eng.embed_templates(enc, np.arange(n), np.arange(n + 1), normalize_rows=True)         # embeddings(norm=True), whitebox.py:778-783
    pairs, base = [], 0
    for m in sizes:
        pairs.append(np.array([[base, base + 1]]))
        for i in (0, 1):
            pairs.append(np.stack([np.full(m, base + i), base + 2 + np.arange(m)], axis=1))
        base += 2 + m
    d = eng.pair_dists(unit, unit, np.concatenate(pairs)).cpu().numpy()
    starts = np.cumsum([0] + [1 + 2 * m for m in sizes[:-1]])
    keep = np.ones(d.size, dtype=bool)
    keep[starts] = False
    return d[starts], d[keep]


def calc_mate_nonmate_dists(net, num_subjects, seed, output_dir, ijbc_path, intake='auto'):
    """Drop-in for net_mate_nonmate_dists.py:55-144: distances of mated pairs and of non-mated pairs over IJB-C, the same metadata filter and the
    same draws in the same order.  -> (mate_dists float32 [S], nonmate_dists float32 [S * 2 * 64])."""
    import pandas as pd
    ijbc_metadata = pd.read_csv(os.path.join(ijbc_path, 'protocols', 'ijbc_metadata.csv'))
    ijbc_metadata = ijbc_metadata.loc[np.invert(np.isnan(ijbc_metadata['SUBJECT_ID']))]          # :62
    ijbc_metadata['Filename'] = [os.path.join(ijbc_path, fn) for fn in ijbc_metadata['FILENAME']]
    ijbc_metadata.rename(inplace=True, columns={'SUBJECT_ID': 'SubjectID', 'FACE_X': 'XMin', 'FACE_Y': 'YMin', 'FACE_WIDTH': 'Width',
                                                'FACE_HEIGHT': 'Height'})
    ijbc_metadata = ijbc_metadata.loc[np.invert(np.isnan(ijbc_metadata['XMin'].values)) & np.invert(np.isnan(ijbc_metadata['YMin'].values)) &
                                      np.invert(np.isnan(ijbc_metadata['Width'].values)) & np.invert(np.isnan(ijbc_metadata['Height'].values))]
    ijbc_metadata = ijbc_metadata.loc[ijbc_metadata['Width'] > 100]                              # :81-82
    os.makedirs(output_dir, exist_ok=True)

    random.seed(seed)
    groups = ijbc_metadata.groupby('SubjectID')
    selected = random.sample(range(len(groups)), num_subjects)
    sampled_groups = [grp for i, grp in enumerate(groups) if i in selected]
    seed += 1
    chosen_frames = []
    for sid, subj_grp in sampled_groups:
        if len(subj_grp) < 2:
            continue
        chosen_subjs = subj_grp.sample(2, random_state=seed)
        seed += 1
        chosen_others = ijbc_metadata.loc[ijbc_metadata['SubjectID'] != sid].sample(NUM_NONMATES, random_state=seed)
        chosen_frames.append(pd.concat([chosen_subjs, chosen_others]))
        seed += 1

    if not _is_native(net):
        mate_dists, nonmate_dists = [], []
        for chosen in chosen_frames:
            d_mate, d_non = _host_dists(net.embeddings(chosen, norm=True))
            mate_dists.append(d_mate)
            nonmate_dists.append(d_non)
        return _stack_dists(mate_dists, nonmate_dists)

    def batches():
        for chosen in chosen_frames:
            images = _network_images(net, chosen, intake)
            yield images[:2], images[2:]
    return mate_nonmate_dists(net, batches())


# ---- threshold and Platt scaling (host) -------------------------------------------------------------------------------------------------
def _roc_counts(mate_dists, nonmate_dists):
    """calculate_net_match_threshold.py:76-82,87: -> (thresholds, fp, tp), the counts as integers.  The reference counts by an N x T comparison
    (2.5 GB at the default 128 000 non-mate distances); the count of d <= t is the place of t behind the last equal element of the sorted d."""
    mate_dists, nonmate_dists = np.asarray(mate_dists), np.asarray(nonmate_dists)
    thresholds = np.concatenate([mate_dists, nonmate_dists])
    thresholds.sort()
    thresholds = np.insert(thresholds, 0, 0)
    thresholds = np.around(thresholds, 4)
    thresholds = np.unique(thresholds)
    fp = np.searchsorted(np.sort(nonmate_dists), thresholds, side='right')
    tp = np.searchsorted(np.sort(mate_dists), thresholds, side='right')
    return thresholds, fp, tp


def match_threshold(mate_dists, nonmate_dists, fmr=1e-4):
    """calculate_net_match_threshold.py:76-88: the distance threshold whose false match rate is nearest to `fmr`.
    -> (thresh, thresholds, fpr, tpr)."""
    thresholds, fp, tp = _roc_counts(mate_dists, nonmate_dists)
    fpr = fp.astype(float) / len(nonmate_dists)
    chosen_index = np.argmin(abs(fpr - fmr))
    thresh = thresholds[chosen_index]
    tpr = tp.astype(float) / len(mate_dists)
    return thresh, thresholds, fpr, tpr


def platt_scaling(mate_dists, nonmate_dists, thresh):
    """calculate_net_match_threshold.py:90-99: alpha of Prob = 1 / (1 + exp(-alpha * (dist - thresh))), the minimiser of sklearn's
    LogisticRegression(fit_intercept=False) objective with C = 1 on the one feature d - thresh, label 1 for non-mates:
        f(w) = w^2 / 2 + sum_i log(1 + exp(-y_i x_i w)),   y_i = -1 (mate), +1 (non-mate)
    f is strictly convex (f'' >= 1), so a damped 1-D Newton iteration in float64 finds its only minimum; no sklearn on the product path."""
    from scipy.special import expit
    mate_dists, nonmate_dists = np.asarray(mate_dists), np.asarray(nonmate_dists)
    dists = np.concatenate([mate_dists, nonmate_dists]) - thresh                                 # :91, in the distances' dtype
    s = dists.astype(np.float64)
    s[:len(mate_dists)] *= -1.0                                                                  # y_i x_i

    def f(w):
        return 0.5 * w * w + np.logaddexp(0.0, -s * w).sum()
    w, fw = 0.0, f(0.0)
    for _ in range(200):
        p = expit(-s * w)
        grad = w - (s * p).sum()
        hess = 1.0 + (s * s * p * (1.0 - p)).sum()
        step = grad / hess
        w_new, f_new = w - step, f(w - step)
        while f_new > fw and abs(step) > 1e-16 * max(1.0, abs(w)):                               # never taken on a convex f but for rounding
            step *= 0.5
            w_new, f_new = w - step, f(w - step)
        done = abs(w_new - w) <= 1e-15 * max(1.0, abs(w_new))
        w, fw = w_new, f_new
        if done:
            break
    return float(w)


def calibrate(wb, mate_dists, nonmate_dists):
    """Sets wb.match_threshold and wb.platts_scaling from the distances (the two lines the reference's script prints, :106-107); returns both."""
    thresh = match_threshold(mate_dists, nonmate_dists)[0]
    alpha = platt_scaling(mate_dists, nonmate_dists, thresh)
    wb.match_threshold = float(thresh)
    wb.platts_scaling = alpha
    return wb.match_threshold, wb.platts_scaling


# ---- separability of the game's triplets ------------------------------------------------------------------------------------------------
def _decide(pr_dist, pg_dist, tpr_dist, tpg_dist, thr):
    """filter_inpaintinggame_for_net.py:157-181 on P x 1 distances."""
    mate_correct = ((pr_dist < pg_dist) & (pr_dist < thr))
    mate_diff = pg_dist - pr_dist
    twin_correct = ((tpg_dist < tpr_dist) & (tpr_dist > thr))
    twin_diff = tpr_dist - tpg_dist
    return mate_correct, mate_diff, twin_correct, twin_diff


def _separability(snet, probe_images, mate_images, masks, intake='auto'):
    """:105-181 with average_nonmates for one subject; masks: a list of (twin probe images, non-mate images).  -> one 4-tuple per mask."""
    thr = snet.match_threshold
    if not _is_native(snet):
        probe_embeds = snet.embeddings(probe_images, norm=True)
        mate_embeds = snet.embeddings(mate_images, norm=True)
        mate_embeds = mate_embeds.mean(axis=0, keepdims=True)
        mate_embeds = mate_embeds / np.linalg.norm(mate_embeds, axis=1, keepdims=True)
        probe_embeds = probe_embeds[:, np.newaxis, :]
        mate_embeds = mate_embeds[:, np.newaxis, :]
        pr_dist = np.linalg.norm(probe_embeds - mate_embeds, axis=2)
        out = []
        for twin_probe_images, nonmate_images in masks:
            twin_probe_embeds = snet.embeddings(twin_probe_images, norm=True)
            twin_probe_embeds = twin_probe_embeds[:, np.newaxis, :]
            nonmate_embeds = snet.embeddings(nonmate_images, norm=True)
            nonmate_embeds = nonmate_embeds[np.newaxis, :, :]
            nonmate_embeds = nonmate_embeds.mean(axis=1, keepdims=True)
            nonmate_embeds = nonmate_embeds / np.linalg.norm(nonmate_embeds, axis=2, keepdims=True)
            pg_dist = np.linalg.norm(probe_embeds - nonmate_embeds, axis=2)
            pg_dist = pg_dist.min(axis=1, keepdims=True)
            tpg_dist = np.linalg.norm(twin_probe_embeds - nonmate_embeds, axis=2)
            tpr_dist = np.linalg.norm(twin_probe_embeds - mate_embeds, axis=2)
            tpg_dist = tpg_dist.min(axis=1, keepdims=True)
            out.append(_decide(pr_dist, pg_dist, tpr_dist, tpg_dist, thr))
        return out
    # one embedding pass: probes, mates, then per mask its twins and its non-mates; templates: every probe and twin alone, the mates and each
    # mask's non-mates as one group each
    probes, mates = _network_images(snet, probe_images, intake), _network_images(snet, mate_images, intake)
    P = len(probes)
    images, offsets = probes + mates, list(range(P + 1)) + [P + len(mates)]
    for twin_probe_images, nonmate_images in masks:
        twins, nonmates = _network_images(snet, twin_probe_images, intake), _network_images(snet, nonmate_images, intake)
        if len(twins) != P:
            raise ValueError('%d twin probes of %d probes' % (len(twins), P))
        base = offsets[-1]
        offsets += list(range(base + 1, base + P + 1)) + [base + P + len(nonmates)]
        images += twins + nonmates
    eng, enc = _device_encodings(snet, images)
    tpl = eng.embed_templates(enc, np.arange(enc.shape[0]), offsets, normalize_rows=True)
    probe_t, mate_t = np.arange(P), P
    pairs = [np.stack([probe_t, np.full(P, mate_t)], axis=1)]
    for k in range(len(masks)):
        twin_t, nonmate_t = P + 1 + k * (P + 1) + np.arange(P), P + 1 + k * (P + 1) + P
        pairs += [np.stack([probe_t, np.full(P, nonmate_t)], axis=1), np.stack([twin_t, np.full(P, nonmate_t)], axis=1),
                  np.stack([twin_t, np.full(P, mate_t)], axis=1)]
    d = eng.pair_dists(tpl, tpl, np.concatenate(pairs)).cpu().numpy().reshape(-1, P, 1)
    return [_decide(d[0], d[1 + 3 * k], d[3 + 3 * k], d[2 + 3 * k], thr) for k in range(len(masks))]


def triplet_separability(snet, probe_images, mate_images, twin_probe_images, nonmate_images, intake='auto'):
    """filter_inpaintinggame_for_net.py:105-181 with average_nonmates=True for one subject and one mask: is every probe nearer to the mean of its
    mates than to the mean of the inpainted non-mates and under snet.match_threshold, and every inpainted twin the other way round.
    -> (mate_correct bool, mate_diff float32, twin_correct bool, twin_diff float32), each P x 1; the differences are positive where separable."""
    return _separability(snet, probe_images, mate_images, [(twin_probe_images, nonmate_images)], intake)[0]


def separability_table(snet, inpaintgame_dir, mask_ids=MASK_IDS, net_name='net', return_subject_data=False, intake='auto'):
    """The reference's `separability` DataFrame (:87-250) of one network over every subj-*.csv of the game's directory, one row per (probe, mask):
    the 13 columns of :236-250, cells as the reference leaves them (CorrectlyCls / OrigTripletSim ... hold arrays of one element).
    return_subject_data: also the concatenated subject tables (`all_subj_data`, :234) that include_masks_by_thresholds takes."""
    import pandas as pd
    inpainting_pattern = os.path.join(inpaintgame_dir, INPAINTING_PATTERN_REL)
    original_pattern = os.path.join(inpaintgame_dir, ORIGINAL_PATTERN_REL)
    all_subj_data, separability = [], []
    for subj_csv_fn in sorted(glob.glob(os.path.join(inpaintgame_dir, 'subj-*.csv'))):
        subj_data = pd.read_csv(subj_csv_fn)
        all_subj_data.append(subj_data)
        subj_data['ORIGINAL_BASENAME'] = [os.path.splitext(fn)[0] for fn in subj_data['ORIGINAL_FILE']]
        rows = [row.to_dict() for _, row in subj_data.iterrows()]
        probe_fns = [original_pattern.format(**d) for d in rows if d['TRIPLET_SET'] == 'PROBE']
        mate_fns = [original_pattern.format(**d) for d in rows if d['TRIPLET_SET'] == 'REF']
        masks = []
        for mask_id in mask_ids:
            twin_probe_fns = [inpainting_pattern.format(**dict(d, MASK_ID=mask_id)) for d in rows if d['TRIPLET_SET'] == 'PROBE']
            nonmate_fns = [inpainting_pattern.format(**dict(d, MASK_ID=mask_id)) for d in rows if d['TRIPLET_SET'] != 'PROBE']
            masks.append((twin_probe_fns, nonmate_fns))
        results = _separability(snet, probe_fns, mate_fns, masks, intake)
        for mask_id, (mate_correct, mate_diff, twin_correct, twin_diff) in zip(mask_ids, results):
            for i, d in enumerate(d for d in rows if d['TRIPLET_SET'] == 'PROBE'):
                d = dict(d, MASK_ID=mask_id)
                separability.append((net_name, d['SUBJECT_ID'], d['ORIGINAL_FILE'], d['ORIGINAL_BASENAME'], d['TRIPLET_SET'], mask_id,
                                     mate_correct[i], mate_diff[i], twin_correct[i], twin_diff[i], ORIGINAL_PATTERN_REL.format(**d),
                                     INPAINTING_PATTERN_REL.format(**d), 'average'))
    separability = pd.DataFrame(separability, columns=SEPARABILITY_COLUMNS)
    if return_subject_data:
        return separability, pd.concat(all_subj_data)
    return separability


def include_masks_by_thresholds(data, all_subj_data):
    """filter_inpaintinggame_for_net.py:261-341: the rows of the filtered-masks table of one network.  A (subject, mask) keeps the probes whose
    original and twin are both classified correctly, and, if any is kept, one row per reference image of the subject."""
    import pandas as pd
    all_columns = ['SUBJECT_ID', 'MASK_ID', 'ORIGINAL_BASENAME', 'OriginalFile', 'InpaintingFile', 'TRIPLET_SET', 'OrigTripletSim_resnet',
                   'TwinTripletSim_resnet', 'OrigTripletSim_vgg', 'TwinTripletSim_vgg']
    included_masks = []
    for (subject_id, mask_id), grp in data.groupby(['SUBJECT_ID', 'MASK_ID']):
        some_probes_added = False
        columns = None
        for keys, grp2 in grp.groupby(['OriginalFile', 'InpaintingFile']):
            accept = np.all([bool(np.all(c)) and bool(np.all(t)) for c, t in zip(grp2['CorrectlyCls'], grp2['TwinCorrectlyCls'])])      # :268-270
            if not accept:
                continue
            some_probes_added = True
            grp2_mean = grp2.iloc[[0]].copy()
            for net in ('resnet', 'vgg'):                                                        # :276-294
                of_net = grp2.loc[grp2['NET'] == net]
                if len(of_net):
                    grp2_mean['OrigTripletSim_' + net] = of_net['OrigTripletSim'].values[0][0]
                    grp2_mean['TwinTripletSim_' + net] = of_net['TwinTripletSim'].values[0][0]
            columns = [col for col in all_columns if col in grp2_mean.keys()]
            included_masks.append(grp2_mean[columns])
        if not some_probes_added:
            continue
        ref_match = all_subj_data.loc[(all_subj_data['SUBJECT_ID'] == subject_id) & (all_subj_data['TRIPLET_SET'] == 'REF')]
        for (_, original_basename), grp2 in ref_match.groupby(['SUBJECT_ID', 'ORIGINAL_BASENAME']):
            df = grp2.copy()
            df['MASK_ID'] = mask_id
            df['OriginalFile'] = ORIGINAL_PATTERN_REL.format(MASK_ID=mask_id, SUBJECT_ID=subject_id, ORIGINAL_BASENAME=original_basename)
            df['InpaintingFile'] = INPAINTING_PATTERN_REL.format(MASK_ID=mask_id, SUBJECT_ID=subject_id, ORIGINAL_BASENAME=original_basename)
            for col in all_columns[6:]:
                df[col] = np.nan
            included_masks.append(df.iloc[[0]][columns])                                         # the columns of the last probe kept, as :338 has them
    return pd.concat(included_masks)


# ---- hard non-mates ---------------------------------------------------------------------------------------------------------------------
def nearest_nonmates(wb, image_chunks, subject_ids, topk):
    """eccv20.py:47-77: one template per subject -- the sum of the raw encodings of its chunk of images, row-normalised -- and for every subject
    the `topk` nearest other subjects in embedding space.  image_chunks: one minibatch tensor (n_i x C x H x W) per subject.
    -> {subject id: [the topk nearest other subject ids, nearest first]}."""
    import torch
    from ._lib import MATCH_MAX_D, MATCH_MAX_K
    subject_ids = list(subject_ids)
    if len(image_chunks) != len(subject_ids):
        raise ValueError('%d chunks of images for %d subjects' % (len(image_chunks), len(subject_ids)))
    k = min(int(topk), len(subject_ids) - 1)
    native = _is_native(wb) and 1 <= k <= MATCH_MAX_K
    if native:
        offsets = np.cumsum([0] + [len(chunk) for chunk in image_chunks])
        eng, enc = _device_encodings(wb, (im for chunk in image_chunks for im in chunk))
        native = enc.shape[1] <= MATCH_MAX_D
    if native:
        X = eng.embed_templates(enc, np.arange(enc.shape[0]), offsets, normalize_rows=False)     # :53-54
        idx, _ = eng.nearest_rows(X, X, k, exclude_same_index=True)                              # :57-58
        nearest = idx.cpu().numpy()
    else:
        from scipy.spatial.distance import pdist, squareform
        X = [torch.squeeze(torch.sum(wb.net.encode(imchunk), dim=0)).detach().cpu().numpy() for imchunk in image_chunks]
        X = np.array(X)
        X = X / np.linalg.norm(X, axis=1, keepdims=True)                                         # vipy.linalg.row_normalized
        nearest = [np.argsort(d)[1:][0:topk] for d in squareform(pdist(X, metric='euclidean'))]
    return {subject_ids[i]: [subject_ids[j] for j in js] for i, js in enumerate(nearest)}


__all__ = ['calc_mate_nonmate_dists', 'mate_nonmate_dists', 'match_threshold', 'platt_scaling', 'calibrate', 'triplet_separability',
           'separability_table', 'include_masks_by_thresholds', 'nearest_nonmates']
