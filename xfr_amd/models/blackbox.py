"""Mirror of python/xfr/models/blackbox.py: STRise blackbox saliency (class STRise, :110-480), with the work around the forward pass on
the device (include/xfr_amd.h: xfr_strise_score / xfr_strise_combine; kernels in csrc/strise.hip).

Same constructor arguments, defaults and error strings, same methods (set_probe, set_black_box, mean_ebp_prior, uniform_prior,
generate_sparse_masks, mask_fill_gray, mask_fill_blur, score_masks, combine_masks, compute_saliency_map, evaluate) and attributes (mask_scores,
saliency_map, prior, original_probe_ref_scores, original_probe_gallery_scores).  What differs from the reference:

* Network.  The network is an xfr_amd Whitebox handed over as `net=`; without it `xfr_amd.create_wbnet` builds one for the two black-box names
  the reference knows ('resnetv4_pytorch', 'resnetv6_pytorch').  It also computes the mean-EBP prior, whose seed is uniform over the network's own
  classes (the reference hard-codes the 65359 of its checkpoint, :291-292).
* Random draws.  generate_sparse_masks draws from the global np.random in exactly the reference's order -- all `choice` calls (:321-323), then the
  (x, y) pairs (:330-332) -- and keeps only `mask_cells` (num_masks x num_mask_elements) and `mask_shifts` (num_masks x 2).  `masks` is a property
  that materialises the float64 masks on request (xfr_strise_debug_masks; 2.6 GB at the defaults).  `masked_probes` is not kept: masked_probe(i).
  The mask law is skimage >= 0.19's order-1 'reflect' resize, i.e. scipy.ndimage.zoom(order=1, mode='mirror', grid_mode=True); parity of that
  restatement, of the prior's two resizes (saliency_io.resize_linear) and of the blur below with a real skimage is UNPINNED -- skimage is not
  available where this was written (STRise section; the same caveat as saliency_io).
* Prior.  The prior's two resizes (to 224 x 224, then to the 19 x 19 grid with anti-aliasing) stay on the host.  uniform_prior sets a constant
  prior, where the reference leaves self.prior unset and then fails in generate_sparse_masks.
* Fill.  The blurred fill is computed once per probe on the host: scipy.ndimage.gaussian_filter(sigma=(s, s, 0), mode='nearest', truncate=4.0) of
  the float64 probe, which is what skimage.filters.gaussian(multichannel=True, preserve_range=True) computes for it.
* Scores.  With a black-box NAME, xfr_strise_score runs the whole sweep: masked probes, forward, similarities and contrastive triplet scores stay on
  the device, in float64 from the fp32 embeddings; masked_probe_ref_scores / masked_probe_gallery_scores are not kept.  The gallery and reference
  embeddings enter un-normalised (the kernel normalises in float64; the reference normalises twice in fp32, :375 and :385).
* Percentile.  np.percentile over the scores stays on the host, bit for bit the reference's; the weights go to xfr_strise_combine.
* User callable.  A `black_box_fn` callable still works: masked probes are produced by the device kernel batch by batch, handed to the callable as
  float64 H x W x 3 arrays (the fp32 network input plus the mean: within 2**-16 of the reference's arrays), and the score rows are concatenated.
* Generator's black box.  WhiteboxBlackBox(wb) as `black_box_fn` is the eval scripts' bb_fn (every masked probe through wb.convert_from_numpy,
  i.e. a uint8 image, and the network's own preprocess) for ResNet-101, ResNet-50-128d and Light-CNN; score_masks runs it as one native sweep
  (xfr_strise_score_ex, quantize = 1; masks by scipy's zoom to the bit, mask_law_scipy) and falls back to the callable itself where
  WhiteboxBlackBox.device_route says so.  `score_route` tells which was taken.
* Progress.  evaluate() runs the reference's five stages in its order and prints one line of its own before each.

Out of scope, as in the issue this implements: potential_gallery / build_gallery (commented out in the reference), the plotting helpers."""
import numpy as np
import torch

from ..image_loader import center_crop
from ..saliency_io import resize_linear
from .resnet import MEAN_RGB
from .whitebox import Whitebox, _is_dataframe



def convert_resnet101v4_image(img):
    """resnet.py:25-37 for an H x W x 3 array."""
    return torch.from_numpy(np.moveaxis(np.asarray(img) - np.asarray(MEAN_RGB), 2, 0)).float()


def mask_law(grid, out_shape, mask_scale, shift):
    """One mask on the host, in float64, by the closed form the kernels evaluate (csrc/strise.hip): `grid` gh x gw, out_shape (H, W), shift (x, y)."""
    grid = np.asarray(grid, dtype=np.float64)

    def taps(n, g, s, sh):
        c = (np.arange(n) + sh + 0.5) * (g / float(n + s)) - 0.5
        i0 = np.floor(c)
        f = c - i0

        def mirror(i):
            if g == 1:
                return np.zeros_like(i, dtype=np.int64)
            p = 2 * (g - 1)
            i = np.abs(i.astype(np.int64)) % p
            return np.where(i > g - 1, p - i, i)
        return mirror(i0), mirror(i0 + 1), f
    r0, r1, fy = taps(out_shape[0], grid.shape[0], mask_scale, shift[0])
    c0, c1, fx = taps(out_shape[1], grid.shape[1], mask_scale, shift[1])
    top = (1.0 - fx) * grid[np.ix_(r0, c0)] + fx * grid[np.ix_(r0, c1)]
    bot = (1.0 - fx) * grid[np.ix_(r1, c0)] + fx * grid[np.ix_(r1, c1)]
    return (1.0 - fy)[:, None] * top + fy[:, None] * bot


def mask_law_scipy(grid, out_shape, mask_scale, shift):
    """One mask on the host in scipy's own arithmetic: scipy.ndimage.zoom(grid, order=1, mode='mirror', grid_mode=True) to
    (H + mask_scale, W + mask_scale), cropped at `shift`, BIT FOR BIT (scipy 1.15.3; csrc/strise.hip's exact_taps / mask_exact are the device
    twin).  Per axis: the coordinate is (k + 0.5) * (g / (n + s)) - 0.5 with a negative coordinate reflected (not the tap indices), the last
    spline weight is one minus the other (w1 = 1 - w0, not the fraction), the upper tap folds at g - 1; the four products are summed from 0.0
    in tap order, rows outermost, each as (G * wy) * wx.  Where mask_law above is 1 this is often 1 - 2**-53, which the quantised black box
    of WhiteboxBlackBox sees as a uint8 level."""
    grid = np.asarray(grid, dtype=np.float64)

    def taps(n, g, sh):
        ratio = g / float(n + mask_scale)
        cc = ((np.arange(n) + sh + 0.5) * ratio) - 0.5
        c = np.where(cc < 0, -cc, cc)
        st = np.floor(c)
        w0 = 1.0 - (c - st)
        w1 = 1.0 - w0
        i0 = st.astype(np.int64)
        i1 = i0 + 1
        i1 = np.where(i1 > g - 1, 2 * (g - 1) - i1, i1)
        if g == 1:
            return np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.ones(n), np.zeros(n)
        return i0, i1, w0, w1
    r0, r1, wy0, wy1 = taps(out_shape[0], grid.shape[0], shift[0])
    c0, c1, wx0, wx1 = taps(out_shape[1], grid.shape[1], shift[1])
    t = 0.0 + (grid[np.ix_(r0, c0)] * wy0[:, None]) * wx0[None, :]
    t = t + (grid[np.ix_(r0, c1)] * wy0[:, None]) * wx1[None, :]
    t = t + (grid[np.ix_(r1, c0)] * wy1[:, None]) * wx0[None, :]
    return t + (grid[np.ix_(r1, c1)] * wy1[:, None]) * wx1[None, :]


PIL_PRECISION_BITS = 22      # Pillow's 8-bit resampling: coefficients in 2**-22, src/libImaging/Resample.c
STRISE_MAX_TAPS = 8          # XFR_STRISE_MAX_TAPS


def pil_bilinear_axis(n_in, n_out):
    """PIL.Image.resize(..., BILINEAR) along one axis of a uint8 image, as integers: (first [n_out], count [n_out], coef [n_out][ksize] int32).
    Output xx is clip8((2**21 + sum_t pixel[first + t] * coef[t]) >> 22)  (Pillow 12's precompute_coeffs / normalize_coeffs_8bpc)."""
    scale = n_in / float(n_out)
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    first = np.zeros(n_out, dtype=np.int32)
    count = np.zeros(n_out, dtype=np.int32)
    coef = np.zeros((n_out, ksize), dtype=np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) * ss)) for x in range(xmax)]
        total = sum(w, 0.0)                                       # Pillow adds the weights one by one, left to right
        first[xx], count[xx] = xmin, xmax
        coef[xx, :xmax] = [int(0.5 + (v / total if total != 0.0 else v) * (1 << PIL_PRECISION_BITS)) for v in w]
    return first, count, coef


def pil_bilinear_tables(probe_hw, resize_short, crop_hw):
    """The two tap tables (rows, columns) of torchvision's Resize(resize_short) + CenterCrop(crop_hw) on a uint8 probe of probe_hw, restated on
    PIL's integer bilinear resize (lightcnn.py:27-31; xfr_amd.models.lightcnn.lightcnn_preprocess): only the outputs the crop keeps.  Each table
    is a dict first [n] int32, count [n] int32, coef [n][ksize] int32; the resize runs its horizontal pass (columns) first, rounded to uint8, then
    the vertical one (rows) -- apply_pil_tables below is the numpy statement.  A table with more than STRISE_MAX_TAPS taps does not fit the
    device path (Engine.strise_* refuses it; STRise.score_masks falls back to the host)."""
    h, w = int(probe_hw[0]), int(probe_hw[1])
    if w <= h:
        nw, nh = int(resize_short), int(resize_short * h / w)
    else:
        nw, nh = int(resize_short * w / h), int(resize_short)
    tabs = []
    for n_in, n_out, n_crop in ((h, nh, int(crop_hw[0])), (w, nw, int(crop_hw[1]))):
        off = int(round((n_out - n_crop) / 2.0))
        if off < 0:
            raise ValueError('pil_bilinear_tables: a crop of %d from %d' % (n_crop, n_out))
        first, count, coef = pil_bilinear_axis(n_in, n_out)
        tabs.append(dict(first=first[off:off + n_crop].copy(), count=count[off:off + n_crop].copy(), coef=coef[off:off + n_crop].copy()))
    return tabs[0], tabs[1]


def apply_pil_tables(img_u8, row_tab, col_tab):
    """uint8 H x W x C image -> the resized and cropped uint8 image of pil_bilinear_tables, in numpy: columns first, rounded, then rows."""
    img = np.asarray(img_u8).astype(np.int64)

    def one_pass(a, tab):      # along axis 0
        out = np.empty((len(tab['first']),) + a.shape[1:], dtype=np.int64)
        for i, (f, n) in enumerate(zip(tab['first'], tab['count'])):
            acc = np.tensordot(tab['coef'][i, :n].astype(np.int64), a[f:f + n], axes=1) + (1 << (PIL_PRECISION_BITS - 1))
            out[i] = np.clip(acc >> PIL_PRECISION_BITS, 0, 255)
        return out
    horiz = one_pass(img.transpose(1, 0, 2), col_tab).transpose(1, 0, 2)
    return one_pass(horiz, row_tab).astype(np.uint8)


BLACK_BOX_NAMES = ('resnetv4_pytorch', 'resnetv6_pytorch')
_COLLECTION = 'a list of filepaths, NumPy arrays, or a Pandas dataframe'


def _is_collection(obj):
    return isinstance(obj, (list, np.ndarray)) or _is_dataframe(obj)


def _choose(table, key, what):
    """table[key], refused in the reference's words: `what` is (message for None, message with one {} for an unknown key)."""
    if key is None:
        raise ValueError(what[0])
    if key not in table:
        raise ValueError(what[1].format(key))
    return table[key]


def _unit_rows(v):
    v = np.asarray(v)
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def l2_similarity(probe_vecs, gallery_vecs):
    """1 - |p / |p| - g / |g|| / 2 for every (probe row, gallery row) pair (:385): len(probe_vecs) x len(gallery_vecs)."""
    gap = _unit_rows(probe_vecs)[:, None, :] - _unit_rows(gallery_vecs)[None, :, :]
    return 1.0 - 0.5 * np.linalg.norm(gap, axis=2)


class WhiteboxBlackBox(object):
    """The generator's black box (eval/generate_inpaintinggame_bb_saliency_maps_multigpu.py:73-101) around an xfr_amd Whitebox: called with
    (probes, gallery) it is that bb_fn line for line -- H x W x 3 arrays through wb.convert_from_numpy, then wb.embeddings, then the L2
    similarity -- and works wherever a user callable does.  STRise.score_masks recognises it and runs the whole sweep natively on wb's engine
    (xfr_strise_score_ex, quantize = 1) where device_route allows."""

    RESIZE_SHORT = 144      # lightcnn.py:28, Resize(144) in front of CenterCrop(in_h x in_w)

    def __init__(self, wb):
        if not isinstance(wb, Whitebox):
            raise ValueError('wb must be an xfr_amd Whitebox')
        self.wb = wb

    def _vectors(self, images):
        if isinstance(images[0], np.ndarray):
            if images[0].shape[2] == 3:                    # "If third channel equals 3, assume images need preprocessing" (:81,88)
                images = [self.wb.convert_from_numpy(im)[0] for im in images]
        return self.wb.embeddings(images)

    def __call__(self, probes, gallery):
        gallery_vecs = self._vectors(gallery)
        probe_vecs = self._vectors(probes)
        return l2_similarity(probe_vecs, gallery_vecs)

    def embed_raw(self, images):
        """Un-normalised fp32 encodings n x D of references / gallery images, through the same conversion."""
        if not _is_dataframe(images) and isinstance(images[0], np.ndarray) and images[0].shape[2] == 3:
            images = [self.wb.convert_from_numpy(im)[0] for im in images]
        v = np.asarray(self.wb.embeddings(images, norm=False))
        return torch.from_numpy(v.reshape(v.shape[0], -1))

    def resample_tables(self, probe_hw):
        """The tap tables of a luminance network's Resize + CenterCrop (pil_bilinear_tables), None for a sub-mean network."""
        spec = self.wb.net.u8_preprocess_spec()
        if spec is None or spec[0] != 'luminance':
            return None
        return pil_bilinear_tables(probe_hw, self.RESIZE_SHORT, self.wb.net.net.in_shape[1:])

    def device_route(self, probe, fill):
        """-> (True, tables or None) where the native sweep computes what __call__ computes, else (False, the reason).  The host path is taken for
        a probe that is not 224 x 224 (convert_from_numpy resizes it, whitebox.py:802); for np.minimum(probe, fill).max() < 2 (the / 255 of
        whitebox.py:794-795 is conditional on the image's maximum exceeding 1, and only this bound guarantees it for every masked probe); for a
        resampling table with more than STRISE_MAX_TAPS taps; for a network without u8_preprocess_spec; and for a sub-mean network whose input is
        not the 224 x 224 that convert_from_numpy produces (xfr_strise_score_ex would refuse it)."""
        if tuple(probe.shape[0:2]) != (224, 224):
            return False, 'the probe is %d x %d, not 224 x 224' % tuple(probe.shape[0:2])
        if np.minimum(probe, fill).max() < 2:
            return False, 'min(probe, fill) stays below 2: the / 255 of convert_from_numpy is not certain'
        spec = self.wb.net.u8_preprocess_spec()
        if spec is None:
            return False, 'the network states no uint8 preprocessing (u8_preprocess_spec)'
        tables = self.resample_tables(probe.shape[0:2])
        if tables is not None and max(int(t['count'].max()) for t in tables) > STRISE_MAX_TAPS:
            return False, 'a resampling table has more than %d taps' % STRISE_MAX_TAPS
        if tables is None and tuple(self.wb.net.net.in_shape[1:]) != (224, 224):
            return False, 'the network input is not 224 x 224'
        return True, tables


class STRise:
    def __init__(self, probe=None, refs=None, ref_sids=None, potential_gallery=None, gallery=None, gallery_size=50, black_box=None,
                 black_box_fn=None, prior_type='mean_ebp', mask_type='sparse', num_mask_elements=1, num_masks=6500, mask_scale=12,
                 mask_fill_type='blur', blur_fill_sigma_percent=4, triplet_score_type='cts', use_gpu=True, device=None, net=None):
        if net is not None and not isinstance(net, Whitebox):
            raise ValueError('net must be an xfr_amd Whitebox')
        self.net, self.use_gpu = net, use_gpu
        self.device = torch.device('cuda') if device is None else device
        self.mean_ebp_net = self.resnet_net = None
        # the reference's lookup tables, under its names (:133-148)
        self.priors = dict(mean_ebp=self.mean_ebp_prior, uniform=self.uniform_prior)
        self.black_boxes = dict.fromkeys(BLACK_BOX_NAMES, self.resnet_bb_fn)
        self.mask_types = dict(sparse=self.generate_sparse_masks)
        self.mask_fill_types = dict(gray=self.mask_fill_gray, blur=self.mask_fill_blur)
        self.triplet_scoring_fns = dict(cts=self.contrastive_triplet_similarity)

        # the checks come in the reference's order, so that a call with several faults fails with the reference's message (:163-261)
        if probe is None or refs is None:
            raise ValueError('Probe and reference must be specified')
        self.probe = self._crop(probe, convert_uint8=True)
        if not _is_collection(refs):
            raise ValueError('Refs must be ' + _COLLECTION)
        self.refs, self.ref_sids = refs, ref_sids
        _choose(self.priors, prior_type, ('Prior must be specified', 'Specified prior "{}" is not supported'))
        self.prior_type = prior_type
        for label, images in (('Potential gallery', potential_gallery), ('Gallery', gallery)):
            if images is not None and not _is_collection(images):
                raise TypeError(label + ' must be ' + _COLLECTION)
        self.potential_gallery = potential_gallery
        if potential_gallery is not None:
            self.potential_gallery_size = len(potential_gallery)
        self.gallery = gallery
        self.gallery_size = gallery_size if gallery is None else len(gallery)
        self.black_box = None
        if black_box:
            self.set_black_box(black_box)
        elif black_box_fn:
            self.black_box_fn = black_box_fn
        else:
            raise ValueError('Black box name or function must be specified')
        self.generate_masks = _choose(self.mask_types, mask_type, ('Mask type must be specified', 'Specified mask type "{}" is not supported'))
        self.mask_type = mask_type
        self.apply_masks = _choose(self.mask_fill_types, mask_fill_type,
                                   ('Mask fill type must be specified', 'Specified mask fill type "{}" is not supported'))
        self.mask_fill_type = mask_fill_type
        self.triplet_scoring_fn = _choose(self.triplet_scoring_fns, triplet_score_type,
                                          ('Triplet score type must be specified', 'Specified triplet score type "{}" is not supported.'))
        self.triplet_score_type = triplet_score_type
        self.num_mask_elements, self.num_masks, self.mask_scale = num_mask_elements, num_masks, mask_scale
        self.blur_fill_sigma_percent = blur_fill_sigma_percent      # sigma of the blurred fill, in percent of the probe's longer side

    # -- plumbing ------------------------------------------------------------------------------------------
    @staticmethod
    def _crop(probe, convert_uint8):
        if not isinstance(probe, (str, np.ndarray)):
            raise ValueError('Probe must be a filepath to an image or a NumPy array')
        return center_crop(probe, convert_uint8=convert_uint8)

    def _network(self):
        """The Whitebox behind the named black box (:367-368 creates it on first use)."""
        if self.resnet_net is None:
            if self.net is not None:
                self.resnet_net = self.net
            else:
                from ..create_wbnet import create_wbnet
                self.resnet_net = create_wbnet(self.black_box or BLACK_BOX_NAMES[0], device=self.device, ebp_version=6)
        return self.resnet_net

    def _engine(self):
        wb = self._network()
        return wb._engine(wb.batch_size), wb.net._mark('encode')

    def _merge_engine(self):
        """The merge takes the probe's size, not the engine's: behind a WhiteboxBlackBox it runs on that network's engine, whatever its input."""
        if isinstance(self.black_box_fn, WhiteboxBlackBox):
            return self.black_box_fn.wb._engine(self.black_box_fn.wb.batch_size)
        return self._engine()[0]

    def _grid(self, shape=None):
        """Cells of the coarse grid along each axis: ceil(size / mask_scale) (:302)."""
        h, w = (self.probe.shape if shape is None else shape)[0:2]
        return (-(-int(h) // self.mask_scale), -(-int(w) // self.mask_scale))

    def _mask_args(self):
        if getattr(self, 'mask_cells', None) is None:
            raise RuntimeError('generate_sparse_masks has not been called')
        return self.mask_cells, self.mask_shifts, self._grid(), self.mask_scale

    def _fill_image(self):
        if getattr(self, 'fill_image', None) is None:
            raise RuntimeError('mask_fill_gray / mask_fill_blur has not been called')
        return self.fill_image

    # -- reference surface ---------------------------------------------------------------------------------
    def set_probe(self, probe):
        probe = self._crop(probe, convert_uint8=False)
        if probe.dtype != np.uint8:
            raise ValueError('the probe must be a uint8 image')     # the reference goes on with a float probe here (:265); the device path is uint8
        self.probe = probe
        self.fill_image = None
        if getattr(self, 'original_probe_gallery_scores', None) is not None:
            self.original_probe_gallery_scores = None               # scores of the probe before belong to that probe (:270-271)

    def set_black_box(self, black_box):
        fn = self.black_boxes.get(black_box)
        if fn is None:
            raise ValueError('Specified black box "{}" is not supported'.format(black_box))
        self.black_box, self.black_box_fn = black_box, fn

    def mean_ebp_prior(self):
        """EBP from a uniform seed over the classes, as a 224 x 224 map (:280-294)."""
        wb = self.mean_ebp_net
        if wb is None:
            if self.net is not None:
                wb = self.net
            else:
                from ..create_wbnet import create_wbnet
                wb = create_wbnet(BLACK_BOX_NAMES[0], device=self.device, ebp_version=None)
            self.mean_ebp_net = wb
        x = convert_resnet101v4_image(self.probe.copy())[None]
        saved, wb.net._classifier = wb.net._classifier, None      # the hooked N-way classifier, as in a freshly created network
        try:
            n = wb.net.num_classes()
            P = wb.ebp(x, torch.full((1, n), 1.0 / float(n), dtype=torch.float32))
        finally:
            wb.net._classifier = saved
        self.prior = resize_linear(np.asarray(P), (224, 224))

    def uniform_prior(self):
        self.prior = np.ones(self.probe.shape[0:2])

    def generate_sparse_masks(self, random_shift=True, order=1):
        """Draws num_mask_elements cells and one shift per mask (:299-336) -- mask_cells, mask_shifts; the masks themselves are never stored."""
        if order != 1:
            raise ValueError('xfr_amd evaluates the order-1 masks only')
        if not random_shift:
            raise NotImplementedError('random_shift=False resizes the grids without the margin (:335); only the shifted masks are built here')
        n, scale = self.num_masks, self.mask_scale
        # cell probabilities: the prior on the coarse grid, its lower half never drawn, the rest in proportion (flat for the uniform prior)
        p = np.array(resize_linear(self.prior, self._grid(self.prior.shape)), dtype=np.float64).ravel()
        p = np.where(p < np.percentile(p, 50.0), 0.0, p)
        if self.prior_type == 'uniform':
            p = (p > 0).astype(np.float64)
        p = p / p.sum()
        # the global np.random stream is consumed as the reference consumes it: every mask's cells first (:321-323), then x and y of every
        # mask (:330-332)
        ids = np.arange(p.size)
        cells = [np.random.choice(ids, self.num_mask_elements, replace=False, p=p) for _ in range(n)]
        shifts = [(np.random.randint(0, scale), np.random.randint(0, scale)) for _ in range(n)]
        self.mask_cells = np.asarray(cells, dtype=np.int32).reshape(n, self.num_mask_elements)
        self.mask_shifts = np.asarray(shifts, dtype=np.int32).reshape(n, 2)
        self.mask_scores = None

    @property
    def masks(self):
        """The float64 masks (num_masks x H x W) of blackbox.py:336, materialised on request through the parity hook."""
        eng, _ = self._engine()
        cells, shifts, grid, scale = self._mask_args()
        step = 256
        return np.concatenate([eng.strise_masks(cells, shifts, grid, scale, i, min(step, len(cells) - i)).cpu().numpy()
                               for i in range(0, len(cells), step)], axis=0)

    def _masked_batch(self, first, count):
        """Masked probes [first, first + count) as the reference's float64 H x W x 3 arrays (:343), from the device kernel."""
        eng, _ = self._engine()
        cells, shifts, grid, scale = self._mask_args()
        x = eng.strise_masked_probes(torch.from_numpy(self.probe), torch.from_numpy(self._fill_image()), cells, shifts, grid, scale, first, count)
        return x.double().permute(0, 2, 3, 1).cpu().numpy() + np.asarray(MEAN_RGB, dtype=np.float64)

    def masked_probe(self, i):
        return self._masked_batch(int(i), 1)[0]

    def apply_masks_using_image(self, image):
        """Keeps the fill; the blend itself (:338-345) happens in the masked-probe kernel."""
        image = np.ascontiguousarray(image, dtype=np.float64)
        if image.shape != self.probe.shape:
            raise ValueError('the fill image must have the probe\'s shape')
        self.fill_image = image

    def mask_fill_gray(self):
        self.apply_masks_using_image(np.full(self.probe.shape, 0.5))

    def mask_fill_blur(self):
        import scipy.ndimage
        sigma = self.blur_fill_sigma_percent / 100.0 * max(self.probe.shape)
        blurred = scipy.ndimage.gaussian_filter(self.probe.astype(np.float64), sigma=(sigma, sigma, 0), mode='nearest', truncate=4.0)
        self.apply_masks_using_image(blurred)

    def _embed(self, images):
        """fp32 encodings (n x D, device) of reference / gallery images: H x W x 3 arrays through convert_resnet101v4_image (:371-375), anything
        else through Whitebox.embeddings."""
        wb = self._network()
        if _is_dataframe(images) or not isinstance(images[0], np.ndarray):
            return torch.from_numpy(np.asarray(wb.embeddings(images))).reshape(len(images), -1)
        ts = [convert_resnet101v4_image(im) if im.shape[2] == 3 else torch.from_numpy(im).float() for im in images]
        x = torch.stack(ts)
        return torch.cat([wb.encode(b.to(wb.net.net.device)).detach() for b in torch.split(x, wb.batch_size, dim=0)], dim=0)

    def resnet_bb_fn(self, probes, gallery):
        """:366-388 as a plain callable: similarity scores len(probes) x len(gallery), in fp32 on the host like the reference."""
        return l2_similarity(self._embed(probes).cpu().numpy(), self._embed(gallery).cpu().numpy())

    def contrastive_triplet_similarity(self):
        """Per mask: how much more the mask costs the probe against its references than against the gallery, averaged over the (broadcast)
        pairs (:390-394)."""
        lost_ref = np.asarray(self.original_probe_ref_scores) - np.asarray(self.masked_probe_ref_scores)
        lost_gal = np.asarray(self.original_probe_gallery_scores) - np.asarray(self.masked_probe_gallery_scores)
        return np.mean(lost_ref - lost_gal, axis=1)

    def score_masks(self):
        if self.black_box is not None and self.black_box_fn == self.black_boxes[self.black_box]:
            # the named black box: one native sweep
            eng, enc = self._engine()
            cells, shifts, grid, scale = self._mask_args()
            refs = self._embed(self.refs)
            gal = self._embed(self.gallery)
            scores, orig = eng.strise_score(torch.from_numpy(self.probe), torch.from_numpy(self._fill_image()), cells, shifts, grid, scale, refs, gal, enc)
            orig = orig.cpu().numpy()
            self.original_probe_ref_scores = orig[None, :refs.shape[0]]
            self.original_probe_gallery_scores = orig[None, refs.shape[0]:]
            self.masked_probe_ref_scores = self.masked_probe_gallery_scores = None
            self.mask_scores = scores.cpu().numpy()
            return
        fn = self.black_box_fn
        self.score_route = 'host'
        if isinstance(fn, WhiteboxBlackBox):
            # the generator's black box: one native sweep of the quantised chain on ITS network (the prior's network is `net`)
            ok, tables = fn.device_route(self.probe, self._fill_image())
            if ok:
                self.score_route = 'device'
                eng, enc = fn.wb._engine(fn.wb.batch_size), fn.wb.net._mark('encode')
                cells, shifts, grid, scale = self._mask_args()
                refs, gal = fn.embed_raw(self.refs), fn.embed_raw(self.gallery)
                scores, orig = eng.strise_score(torch.from_numpy(self.probe), torch.from_numpy(self._fill_image()), cells, shifts, grid, scale, refs, gal,
                                                enc, probe_shape=self.probe.shape[0:2], quantize=True, tables=tables)
                orig = orig.cpu().numpy()
                self.original_probe_ref_scores = orig[None, :refs.shape[0]]
                self.original_probe_gallery_scores = orig[None, refs.shape[0]:]
                self.masked_probe_ref_scores = self.masked_probe_gallery_scores = None
                self.mask_scores = scores.cpu().numpy()
                return
            self.score_route = 'host: ' + tables
        # a user callable (:396-414): masked probes batch by batch from the device kernel; the probe's gallery scores survive from an earlier
        # call unless set_probe dropped them
        self.original_probe_ref_scores = fn([self.probe], self.refs)
        if getattr(self, 'original_probe_gallery_scores', None) is None:
            self.original_probe_gallery_scores = fn([self.probe], self.gallery)
        eng, _ = self._engine()
        rows_ref, rows_gal = [], []
        for i in range(0, self.num_masks, eng.max_batch):
            batch = list(self._masked_batch(i, min(eng.max_batch, self.num_masks - i)))
            rows_ref.append(np.asarray(fn(batch, self.refs)))
            rows_gal.append(np.asarray(fn(batch, self.gallery)))
        self.masked_probe_ref_scores = np.concatenate(rows_ref, axis=0)
        self.masked_probe_gallery_scores = np.concatenate(rows_gal, axis=0)
        self.mask_scores = self.triplet_scoring_fn()

    def combine_masks(self, indices):
        """Mean over the selected masks of score x mask (:416-421) on the materialised masks, in numpy: the parity path
        (compute_saliency_map merges on the device)."""
        w = np.asarray(self.mask_scores, dtype=np.float64)[indices]
        return np.tensordot(w, self.masks[indices], axes=1) / len(w)

    def select_masks(self, positive_scores=True, percentile=0):
        """The selection of :424-437 on the host: (boolean array over the masks, sign of the branch).  With the scores of the other sign
        negated, either branch keeps what reaches the given percentile of the positive values; np.percentile does not depend on the order
        of its input, so the threshold is the reference's to the bit."""
        sign = 1 if positive_scores else -1
        signed = sign * np.asarray(self.mask_scores)
        return signed >= np.percentile(signed[signed > 0], percentile), sign

    def compute_saliency_map(self, positive_scores=True, percentile=0):
        selected_indices, sign = self.select_masks(positive_scores, percentile)
        self.selected_indices = selected_indices
        eng = self._merge_engine()
        cells, shifts, grid, scale = self._mask_args()
        weights = np.where(selected_indices, self.mask_scores, 0.0)
        self.saliency_map = eng.strise_combine(weights, int(selected_indices.sum()), cells, shifts, grid, scale, sign,
                                               probe_shape=self.probe.shape[0:2]).cpu().numpy()

    def evaluate(self):
        """Prior, masks, fill, scores, map (:450-479), with a line of progress before each."""
        stages = (('prior', self.priors[self.prior_type]), ('masks', self.generate_masks), ('fill', self.apply_masks),
                  ('scores', self.score_masks), ('saliency map', self.compute_saliency_map))
        for i, (name, run) in enumerate(stages, 1):
            print('STRise %d/%d: %s' % (i, len(stages), name), flush=True)
            run()


__all__ = ['STRise', 'WhiteboxBlackBox', 'mask_law', 'mask_law_scipy', 'pil_bilinear_tables', 'apply_pil_tables', 'convert_resnet101v4_image', 'l2_similarity', 'BLACK_BOX_NAMES']
