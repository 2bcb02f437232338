"""Python handle on one HIP engine (one backbone, one device).  PyTorch tensors are only the container for
device memory and the source of the HIP stream; all arithmetic happens inside libxfr_amd.so."""
import ctypes

import numpy as np
import torch

from . import _lib
from .program import LAYER_NAMES, OpKind

MODES = {'affineonly': 0, 'affineonly_with_prior': 1, 'norelu': 2, 'all': 3}


def _tap_array(tab):
    """One table of xfr_amd.models.blackbox.pil_bilinear_tables (first, count, coef) as an array of xfr_strise_tap."""
    n = len(tab['first'])
    coef = np.asarray(tab['coef'], dtype=np.int32).reshape(n, -1)
    if coef.shape[1] > _lib.STRISE_MAX_TAPS and (coef[:, _lib.STRISE_MAX_TAPS:] != 0).any():
        raise ValueError('a resampling table with more than %d taps' % _lib.STRISE_MAX_TAPS)
    arr = (_lib.StriseTap * n)()
    for i in range(n):
        arr[i].first, arr[i].count = int(tab['first'][i]), int(tab['count'][i])
        for j, v in enumerate(coef[i, :_lib.STRISE_MAX_TAPS]):
            arr[i].coef[j] = int(v)
    return arr


def _stream_ptr(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class Engine(object):
    def __init__(self, program, max_batch, device):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError('xfr_amd: no HIP device visible; the engine has no CPU fallback')
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('xfr_amd: the engine runs on a HIP device, got %s' % (device,))
        if self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        self.program = program
        self.max_batch = int(max_batch)
        self._h = ctypes.c_void_p()
        ops = program.op_array()
        c, h, w = program.in_shape
        _lib.check(self.lib.xfr_engine_create(ops, len(program.ops), len(program.weight_names), c, h, w,
                                              self.max_batch, self.device.index, ctypes.byref(self._h)))
        self._mode = None
        self.loaded_version = None
        self._pipeline = 0
        self.options = {}          # engine-level switches set through this handle (re-applied when a wrapper rebuilds the engine)

    def close(self):
        if getattr(self, '_h', None) is not None and self._h.value:
            self.lib.xfr_engine_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------------------------------------
    def load_weights(self, state_dict):
        names = self.program.weight_names
        views = (_lib.TensorView * len(names))()
        keep = []
        for i, n in enumerate(names):
            if n not in state_dict:
                raise KeyError('xfr_amd: parameter "%s" missing from the state_dict' % n)
            t = state_dict[n].detach().to('cpu', torch.float32).contiguous()
            keep.append(t)
            views[i].data = t.data_ptr()
            views[i].numel = t.numel()
        _lib.check(self.lib.xfr_engine_load_weights(self._h, views, len(names)))

    def weight_arena(self):
        """The packed parameter arena as a uint8 CUDA tensor view (for torch.distributed.broadcast)."""
        p = ctypes.c_void_p()
        nbytes = ctypes.c_size_t()
        _lib.check(self.lib.xfr_engine_weight_arena(self._h, ctypes.byref(p), ctypes.byref(nbytes)))

        class _Arr(object):
            pass
        a = _Arr()
        a.__cuda_array_interface__ = {'shape': (nbytes.value,), 'typestr': '|u1', 'data': (p.value, False),
                                      'version': 2}
        with torch.cuda.device(self.device):
            t = torch.as_tensor(a, device=self.device)
        return t

    def mark_weights_loaded(self):
        _lib.check(self.lib.xfr_engine_mark_weights_loaded(self._h))

    def set_mode(self, subtree_mode, eps=1e-16, with_bias=False):
        if subtree_mode not in MODES:
            raise ValueError('Invalid subtree mode "%s"' % subtree_mode)
        key = (subtree_mode, float(eps), bool(with_bias))
        if key != self._mode:
            _lib.check(self.lib.xfr_engine_set_mode(self._h, MODES[subtree_mode], float(eps), 1 if with_bias else 0))
            self._mode = key

    def tensor_shape(self, tid):
        c, h, w = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        _lib.check(self.lib.xfr_engine_tensor_shape(self._h, int(tid), ctypes.byref(c), ctypes.byref(h), ctypes.byref(w)))
        return (c.value, h.value, w.value)

    def memory(self):
        a, b = ctypes.c_size_t(), ctypes.c_size_t()
        _lib.check(self.lib.xfr_engine_memory(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    # ------------------------------------------------------------------------------------------------
    def _prep(self, x):
        """-> (device tensor, fresh).  fresh: the tensor was produced here (host-to-device copy, cast, .contiguous()), i.e. it
        is still pending on the current stream; such an input must never be declared inputs_ready to the engine, whose
        pipelined forwards run on internal streams that do not wait for the caller's stream."""
        if x.dim() != 4 or tuple(x.shape[1:]) != tuple(self.program.in_shape):
            raise ValueError('expected input N x %s, got %s' % (self.program.in_shape, tuple(x.shape)))
        if x.shape[0] > self.max_batch:
            raise ValueError('batch %d exceeds the engine max_batch %d' % (x.shape[0], self.max_batch))
        y = x.detach().to(self.device, torch.float32).contiguous()
        fresh = (not x.is_cuda) or y.data_ptr() != x.data_ptr()
        return y, fresh

    def _declare_ready(self, ready):
        """Pipeline level 2: tell the engine whether the NEXT ebp / contrastive call may read x without waiting for the
        caller's stream (xfr_engine_set_inputs_ready; the engine consumes the promise with that call, so ebp_capture /
        ebp_firing / layerwise, which never declare anything, always take the safe ordering)."""
        if self._pipeline & 2:
            _lib.check(self.lib.xfr_engine_set_inputs_ready(self._h, 1 if ready else 0))

    def forward(self, x, tensor_id):
        x, _ = self._prep(x)
        c, h, w = self.tensor_shape(tensor_id)
        out = torch.empty((x.shape[0], c, h, w), device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.xfr_forward(self._h, x.data_ptr(), x.shape[0], int(tensor_id), out.data_ptr(),
                                            _stream_ptr(self.device)))
        return out

    def ebp(self, x, seed_tensor, seed, want_mwp=False, want_pooled=True, inputs_ready=False):
        """seed: S x N x D.  Returns (mwp S x N x C1 x H1 x W1 or None, pooled S x N x H1 x W1 or None).
        inputs_ready (pipeline level 2 only): x is resident and valid on the device, see set_pipeline."""
        x, fresh = self._prep(x)
        self._declare_ready(inputs_ready and not fresh)
        n = x.shape[0]
        seed = seed.detach().to(self.device, torch.float32).contiguous()
        S = seed.shape[0]
        d = int(np.prod(self.tensor_shape(seed_tensor)))
        if seed.dim() != 3 or seed.shape[1] != n or seed.shape[2] != d:
            raise ValueError('seed must be S x %d x %d, got %s' % (n, d, tuple(seed.shape)))
        c1, h1, w1 = self.tensor_shape(1)
        mwp = torch.empty((S, n, c1, h1, w1), device=self.device) if want_mwp else None
        pooled = torch.empty((S, n, h1, w1), device=self.device) if want_pooled else None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.xfr_ebp(self._h, x.data_ptr(), n, S, int(seed_tensor), seed.data_ptr(),
                                        mwp.data_ptr() if want_mwp else None,
                                        pooled.data_ptr() if want_pooled else None, _stream_ptr(self.device)))
        return mwp, pooled

    def contrastive(self, x, seed_tensor, seed, percentile=None, raw=False, inputs_ready=False, tail='v6'):
        """seed: 2 x N x D (mate, non-mate).  Returns N x H1 x W1 saliency maps (raw=True: the contrastive MWP before
        _mwp_to_saliency; tail='u8': the uint8 maps of ebp_version != 6, xfr_contrastive_u8)."""
        if tail not in ('v6', 'u8') or (raw and tail != 'v6'):
            raise ValueError("tail must be 'v6' or 'u8' (and 'v6' with raw=True), got %r" % (tail,))
        x, fresh = self._prep(x)
        self._declare_ready(inputs_ready and not fresh)
        n = x.shape[0]
        seed = seed.detach().to(self.device, torch.float32).contiguous()
        d = int(np.prod(self.tensor_shape(seed_tensor)))
        if tuple(seed.shape) != (2, n, d):
            raise ValueError('seed must be 2 x %d x %d, got %s' % (n, d, tuple(seed.shape)))
        c1, h1, w1 = self.tensor_shape(1)
        sal = torch.empty((n, h1, w1), device=self.device, dtype=torch.uint8 if tail == 'u8' else torch.float32)
        pct = -1.0 if percentile is None else float(percentile)
        with torch.cuda.device(self.device):
            fn = self.lib.xfr_contrastive_raw if raw else (self.lib.xfr_contrastive_u8 if tail == 'u8' else self.lib.xfr_contrastive)
            _lib.check(fn(self._h, x.data_ptr(), n, int(seed_tensor), seed.data_ptr(), pct, sal.data_ptr(), _stream_ptr(self.device)))
        return sal

    def triplet_contrastive(self, probes, gallery, encode_tensor, scale=1.0 / 2500.0, percentile=None, inputs_ready=False, tail='v6'):
        """probes N x C x H x W, gallery 2N x C x H x W (mates then non-mates) -> N x H1 x W1 saliency maps (tail='u8': the uint8 maps of
        ebp_version != 6, xfr_triplet_contrastive_u8tail).
        inputs_ready=True: both tensors are already valid on the device (not pending on the current stream) and will not be
        modified or freed until the result has been consumed -- required for cross-call pipelining (set_pipeline)."""
        if tail not in ('v6', 'u8'):
            raise ValueError("tail must be 'v6' or 'u8', got %r" % (tail,))
        probes, fresh = self._prep(probes)
        n = probes.shape[0]
        g_in = gallery
        gallery = gallery.detach().to(self.device, torch.float32).contiguous()
        if fresh or (not g_in.is_cuda) or gallery.data_ptr() != g_in.data_ptr():
            inputs_ready = False          # a copy made here is still pending on the current stream
        if tuple(gallery.shape) != (2 * n,) + tuple(self.program.in_shape):
            raise ValueError('gallery must be %d x %s, got %s' % (2 * n, self.program.in_shape, tuple(gallery.shape)))
        c1, h1, w1 = self.tensor_shape(1)
        sal = torch.empty((n, h1, w1), device=self.device, dtype=torch.uint8 if tail == 'u8' else torch.float32)
        pct = -1.0 if percentile is None else float(percentile)
        with torch.cuda.device(self.device):
            fn = self.lib.xfr_triplet_contrastive_u8tail if tail == 'u8' else self.lib.xfr_triplet_contrastive
            _lib.check(fn(self._h, probes.data_ptr(), gallery.data_ptr(), n, int(encode_tensor), float(scale), pct, sal.data_ptr(),
                          _stream_ptr(self.device), 1 if inputs_ready else 0))
        return sal

    # -- uint8 inputs (include/xfr_amd.h: xfr_forward_u8 / xfr_triplet_contrastive_u8) ---------------------------------
    def set_u8_preprocess(self, kind, channels=3, mean=None, weight=None):
        """kind 'sub_mean' (mean per channel; ResNet-101 / ResNet-50-128d) or 'luminance' (weights per channel of value / 255; Light-CNN)."""
        p = _lib.U8Preprocess()
        p.kind = {'sub_mean': 0, 'luminance': 1}[kind]
        p.channels = int(channels)
        for i, v in enumerate(mean or ()):
            p.mean[i] = float(v)
        for i, v in enumerate(weight or ()):
            p.weight[i] = float(v)
        _lib.check(self.lib.xfr_engine_set_u8_preprocess(self._h, ctypes.byref(p)))
        self._u8_channels = int(channels)
        self.options['u8_preprocess'] = (kind, int(channels), tuple(mean or ()), tuple(weight or ()))

    def _prep_u8(self, x):
        """uint8 N x H x W x C (as decoded) -> (device tensor, fresh); see _prep."""
        c, h, w = self.program.in_shape
        if x.dtype != torch.uint8 or x.dim() != 4 or tuple(x.shape[1:]) != (h, w, getattr(self, '_u8_channels', 3)):
            raise ValueError('expected uint8 images N x %d x %d x %d, got %s %s' % (h, w, getattr(self, '_u8_channels', 3), x.dtype, tuple(x.shape)))
        if x.shape[0] > self.max_batch:
            raise ValueError('batch %d exceeds the engine max_batch %d' % (x.shape[0], self.max_batch))
        y = x.detach().to(self.device, non_blocking=True).contiguous()
        return y, (not x.is_cuda) or y.data_ptr() != x.data_ptr()

    def preprocess_u8(self, x):
        """The fp32 network input (N x C x H x W) the uint8 path builds: parity hook for the reference's preprocess functions."""
        x, _ = self._prep_u8(x)
        out = torch.empty((x.shape[0],) + tuple(self.program.in_shape), device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.xfr_debug_u8_preprocess(self._h, x.data_ptr(), x.shape[0], out.data_ptr(), _stream_ptr(self.device)))
        return out

    def forward_u8(self, x, tensor_id):
        x, _ = self._prep_u8(x)
        c, h, w = self.tensor_shape(tensor_id)
        out = torch.empty((x.shape[0], c, h, w), device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.xfr_forward_u8(self._h, x.data_ptr(), x.shape[0], int(tensor_id), out.data_ptr(), _stream_ptr(self.device)))
        return out

    def triplet_contrastive_u8(self, probes, gallery, encode_tensor, scale=1.0 / 2500.0, percentile=None, inputs_ready=False):
        """triplet_contrastive on uint8 N x H x W x C probes and 2N gallery images (mates then non-mates)."""
        probes, f1 = self._prep_u8(probes)
        gallery, f2 = self._prep_u8(gallery)
        n = probes.shape[0]
        if gallery.shape[0] != 2 * n:
            raise ValueError('gallery must hold %d images, got %d' % (2 * n, gallery.shape[0]))
        c1, h1, w1 = self.tensor_shape(1)
        sal = torch.empty((n, h1, w1), device=self.device)
        pct = -1.0 if percentile is None else float(percentile)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.xfr_triplet_contrastive_u8(self._h, probes.data_ptr(), gallery.data_ptr(), n, int(encode_tensor), float(scale), pct,
                                                           sal.data_ptr(), _stream_ptr(self.device), 1 if (inputs_ready and not f1 and not f2) else 0))
        return sal

    def triplet_contrastive_u8_host(self, probes, gallery, encode_tensor, scale=1.0 / 2500.0, percentile=None):
        """triplet_contrastive on uint8 images in HOST memory (N x H x W x C probes, 2N gallery images; pinned tensors preferably): the engine copies them
        on its own stream into its own staging buffers, so with set_pipeline on the copy and the forwards of this call overlap the previous call's sweep
        (include/xfr_amd.h: xfr_triplet_contrastive_u8_host).  The copy is asynchronous: call wait_inputs_copied() before rewriting the host tensors."""
        c, h, w = self.program.in_shape
        ch = getattr(self, '_u8_channels', 3)
        for x in (probes, gallery):
            if x.is_cuda or x.dtype != torch.uint8 or x.dim() != 4 or tuple(x.shape[1:]) != (h, w, ch) or not x.is_contiguous():
                raise ValueError('expected contiguous uint8 HOST images N x %d x %d x %d, got %s %s on %s' % (h, w, ch, x.dtype, tuple(x.shape), x.device))
        n = probes.shape[0]
        if gallery.shape[0] != 2 * n:
            raise ValueError('gallery must hold %d images, got %d' % (2 * n, gallery.shape[0]))
        if 2 * n > self.max_batch:
            raise ValueError('batch %d exceeds the engine max_batch %d' % (2 * n, self.max_batch))
        c1, h1, w1 = self.tensor_shape(1)
        sal = torch.empty((n, h1, w1), device=self.device)
        pct = -1.0 if percentile is None else float(percentile)
        self._host_inputs = (probes, gallery)        # keep them alive until the next call replaces them (the copy is asynchronous)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.xfr_triplet_contrastive_u8_host(self._h, probes.data_ptr(), gallery.data_ptr(), n, int(encode_tensor), float(scale), pct,
                                                                sal.data_ptr(), _stream_ptr(self.device)))
        return sal

    def wait_inputs_copied(self):
        """Block until the host-to-device copies of the last triplet_contrastive_u8_host call are done (its host tensors may then be rewritten)."""
        _lib.check(self.lib.xfr_engine_wait_inputs_copied(self._h))

    def set_pipeline(self, on):
        """Let the forward of triplet call i+1 overlap the backward of call i (see include/xfr_amd.h for the contract)."""
        _lib.check(self.lib.xfr_engine_set_pipeline(self._h, int(on)))     # 0 off, 1 triplet calls, 2 every run call; | 4: three forward slots
        self._pipeline = int(on)
        self.options['pipeline'] = int(on)

    def set_epilogue_fusion(self, on):
        """Hook chains / BatchNorm+add+ReLU inside the GEMM epilogue (default on) or as their own launches."""
        level = int(on) if not isinstance(on, bool) else (3 if on else 0)      # 0 off, 3 default (1: without the probe forward's BatchNorm / ReLU)
        _lib.check(self.lib.xfr_engine_set_epilogue_fusion(self._h, level))
        self.options['epilogue_fusion'] = level

    def hold_forward(self, on):
        """Consecutive calls on the same input tensor share one forward pass while held (include/xfr_amd.h)."""
        # re-entrant: nested holders (run_jobs_batched around weighted_subtree_ebp) keep one group open
        self._hold_depth = max(0, getattr(self, '_hold_depth', 0) + (1 if on else -1))
        if (on and self._hold_depth == 1) or (not on and self._hold_depth == 0):
            _lib.check(self.lib.xfr_engine_hold_forward(self._h, int(bool(on))))

    def set_tail_balance(self, on):
        """GEMM tail balancing (default on); off = batch-invariant fp32 arithmetic (include/xfr_amd.h)."""
        _lib.check(self.lib.xfr_engine_set_tail_balance(self._h, int(bool(on))))
        self.options['tail_balance'] = bool(on)

    def set_forward_split(self, on):
        """Forward-only batches of >= 32 images as two half batches on the internal streams (default on; include/xfr_amd.h)."""
        _lib.check(self.lib.xfr_engine_set_forward_split(self._h, int(bool(on))))
        self.options['forward_split'] = bool(on)

    def set_lean(self, on):
        """The lean schedule of un-observed sweeps (default on): stored hook quotients / one-bit gates instead of the literal hook operands;
        off = the literal expressions of whitebox.py:388-428 everywhere (include/xfr_amd.h)."""
        _lib.check(self.lib.xfr_engine_set_lean(self._h, int(bool(on))))
        self.options['lean'] = bool(on)

    def set_split_gemm(self, mode):
        """bf16x6 GEMMs for the deep-K stride-1 convolutions (include/xfr_amd.h, conv_gemm_split.hip K17): 0 / False off, 1 / True the forward
        convolutions, 2 the sweep's backward-data GEMMs, 3 both (the default); + 4: whatever the launch's grid (by default launches of fewer than 128
        tiles stay on the fp32 kernels)."""
        mode = int(mode)
        _lib.check(self.lib.xfr_engine_set_split_gemm(self._h, mode))
        self.options['split_gemm'] = mode

    def split_gemm_launches(self):
        """Launches of the bf16x6 kernel so far (process-wide)."""
        n = ctypes.c_int64(0)
        _lib.check(self.lib.xfr_engine_split_gemm_stats(self._h, ctypes.byref(n)))
        return int(n.value)

    def lean_launches(self):
        """Convolution launches of this engine that took the lean (dual-accumulator) form so far."""
        n = ctypes.c_int64(0)
        _lib.check(self.lib.xfr_engine_lean_stats(self._h, ctypes.byref(n)))
        return int(n.value)

    def apply_options(self, options):
        """Re-apply switches recorded by another Engine handle (WhiteboxNetwork.engine rebuilds engines that are too small)."""
        if 'tail_balance' in options:
            self.set_tail_balance(options['tail_balance'])
        if 'forward_split' in options:
            self.set_forward_split(options['forward_split'])
        if 'lean' in options:
            self.set_lean(options['lean'])
        if 'split_gemm' in options:
            self.set_split_gemm(options['split_gemm'])
        if 'u8_preprocess' in options:
            k, c, m, w = options['u8_preprocess']
            self.set_u8_preprocess(k, c, m, w)
        if 'epilogue_fusion' in options:
            self.set_epilogue_fusion(options['epilogue_fusion'])
        if options.get('pipeline'):
            self.set_pipeline(options['pipeline'])

    def mwp_to_saliency(self, pooled):
        pooled = pooled.detach().to(self.device, torch.float32).contiguous()
        n, h, w = pooled.shape
        out = torch.empty_like(pooled)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.xfr_mwp_to_saliency(self._h, pooled.data_ptr(), n, h, w, out.data_ptr(),
                                                    _stream_ptr(self.device)))
        return out

    def mwp_to_saliency_u8(self, t):
        """_mwp_to_saliency of ebp_version != 6 (xfr_mwp_to_saliency_u8: uint8 stretch, Pillow's GaussianBlur(2), uint8 stretch) of N x H x W
        maps -- float32 maps, or uint8 levels, which take NumPy's float64 form of the first stretch -> uint8 device tensor N x H x W.  Chunked
        like the callers of mwp_to_saliency chunk: 2 x max_batch maps a call."""
        t = t.detach()
        if t.dtype != torch.uint8:
            t = t.to(torch.float32)
        t = t.to(self.device).contiguous()
        if t.dim() != 3:
            raise ValueError('expected maps as N x H x W, got %s' % (tuple(t.shape),))
        n, h, w = t.shape
        out = torch.empty((n, h, w), device=self.device, dtype=torch.uint8)
        cap = max(1, 2 * self.max_batch)
        with torch.cuda.device(self.device):
            for i in range(0, max(n, 1), cap):
                m = min(cap, n - i)
                p = t[i:i + m].data_ptr() if m > 0 else None
                f, b = (None, p) if t.dtype == torch.uint8 else (p, None)
                _lib.check(self.lib.xfr_mwp_to_saliency_u8(self._h, f, b, m, h, w, out[i:i + m].data_ptr() if m > 0 else None,
                                                           _stream_ptr(self.device)))
        return out

    def contrast_tail(self, P, percentile=None):
        """Parity hook (xfr_debug_contrast_tail): the tail of contrastive(raw=True) on the caller's P, C x 2N x HW float32 in the engine's internal
        layout (rows 0 .. N-1 the mate sweep, N .. 2N-1 the non-mate sweep) -> (sums 2N float64, thr N float32 or None for the plain contrastive
        form, contrast N x HW)."""
        P = P.detach().to(self.device, torch.float32).contiguous()
        if P.dim() != 3 or P.shape[1] % 2:
            raise ValueError('expected P as C x 2N x HW, got %s' % (tuple(P.shape),))
        c, n, hw = P.shape[0], P.shape[1] // 2, P.shape[2]
        sums = torch.empty((2 * n,), device=self.device, dtype=torch.float64)
        thr = None if percentile is None else torch.empty((n,), device=self.device, dtype=torch.float32)
        out = torch.empty((n, hw), device=self.device, dtype=torch.float32)
        pct = -1.0 if percentile is None else float(percentile)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.xfr_debug_contrast_tail(self._h, P.data_ptr(), c, n, hw, pct, sums.data_ptr(), None if thr is None else thr.data_ptr(),
                                                        out.data_ptr(), _stream_ptr(self.device)))
        return sums, thr, out

    # -- "next" row: layerwise / weighted-subtree EBP ---------------------------------------------------
    def firing_count(self, seed_tensor):
        n = ctypes.c_int32()
        _lib.check(self.lib.xfr_firing_count(self._h, int(seed_tensor), ctypes.byref(n)))
        return n.value

    def firing_names(self, seed_tensor):
        """Class names of the hooked modules in firing order (Whitebox.P_layername without the argument lists)."""
        nf = self.firing_count(seed_tensor)
        kinds = (ctypes.c_int32 * max(nf, 1))()
        _lib.check(self.lib.xfr_firing_kinds(self._h, int(seed_tensor), kinds, nf))
        return [LAYER_NAMES[OpKind(k)] for k in list(kinds)[:nf]]

    def subtree_weights(self, x, seed_tensor, seed, gate_ge0=True):
        """seed 2 x N x D -> (w [n_firings, N] float32, idx [n_firings, N] int32)."""
        x, _ = self._prep(x)
        n = x.shape[0]
        seed = seed.detach().to(self.device, torch.float32).contiguous()
        nf = self.firing_count(seed_tensor)
        w = (ctypes.c_float * (nf * n))()
        idx = (ctypes.c_int32 * (nf * n))()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.xfr_subtree_weights(self._h, x.data_ptr(), n, int(seed_tensor), seed.data_ptr(), 1 if gate_ge0 else 0,
                                                    w, idx, nf * n, _stream_ptr(self.device)))
        return (np.frombuffer(w, dtype=np.float32).reshape(nf, n).copy(), np.frombuffer(idx, dtype=np.int32).reshape(nf, n).copy())

    def ebp_capture(self, x, seed_tensor, seed, elems):
        """N images, seed 1 x N x D; elems[k][b] = flattened (c,h,w) element of firing k for image b (a flat list of n_firings
        ints is accepted for N = 1) -> float32 [n_firings, N] of P[k][b].flatten()[elems[k][b]]."""
        x, _ = self._prep(x)
        n = x.shape[0]
        seed = seed.detach().to(self.device, torch.float32).contiguous()
        nf = self.firing_count(seed_tensor)
        el_np = np.ascontiguousarray(np.asarray(elems, dtype=np.int32).reshape(nf, n))
        out = np.zeros((nf, n), dtype=np.float32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.xfr_ebp_capture(self._h, x.data_ptr(), n, int(seed_tensor), seed.data_ptr(),
                                                el_np.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                                out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), nf, _stream_ptr(self.device)))
        return out if n > 1 else out[:, 0]

    def layerwise(self, x, seed_tensor, firings, elems=None, vals=None, dense_prior=None):
        """Layerwise sweeps of N images sharing their forwards -> pooled P[-2].
        One image: `firings` is a list of J firings (any order) -> J x H1 x W1, in the order given.
        N images: `firings` / `elems` / `vals` are J x N arrays (firing < 0: idle sweep) -> J x N x H1 x W1; hand the sweeps of
        every image over in ascending firing order so that sweep j joins the backward pass where its first prior fires."""
        x, _ = self._prep(x)
        n = x.shape[0]
        f_np = np.asarray(firings, dtype=np.int32)
        if f_np.ndim == 1 and n == 1 and dense_prior is None:
            order = np.argsort(f_np, kind='stable')
            out = self.layerwise(x, seed_tensor, f_np[order].reshape(-1, 1), np.asarray(elems, dtype=np.int32)[order].reshape(-1, 1),
                                 np.asarray(vals, dtype=np.float32)[order].reshape(-1, 1))
            inv = np.empty_like(order)
            inv[order] = np.arange(len(order))
            return out[torch.as_tensor(inv, device=out.device), 0]
        f_np = np.ascontiguousarray(f_np.reshape(-1, n))
        J = f_np.shape[0]
        c1, h1, w1 = self.tensor_shape(1)
        out = torch.empty((J, n, h1, w1), device=self.device)
        el = va = dp = None
        if dense_prior is not None:
            dense_prior = dense_prior.detach().to(self.device, torch.float32).contiguous()
            dp = dense_prior.data_ptr()
        else:
            el_np = np.ascontiguousarray(np.asarray(elems, dtype=np.int32).reshape(J, n))
            va_np = np.ascontiguousarray(np.asarray(vals, dtype=np.float32).reshape(J, n))
            el = el_np.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
            va = va_np.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        with torch.cuda.device(self.device):
            _lib.check(self.lib.xfr_layerwise_ebp(self._h, x.data_ptr(), n, J, int(seed_tensor),
                                                  f_np.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), el, va, dp, out.data_ptr(),
                                                  _stream_ptr(self.device)))
        return out if (n > 1 or dense_prior is None) else out[:, 0]

    SUBTREE_OUTPUTS = {'mwp': _lib.SUBTREE_MWP, 'saliency': _lib.SUBTREE_SALIENCY, 'uint8': _lib.SUBTREE_UINT8,
                       'uint8_saliency': _lib.SUBTREE_UINT8_SALIENCY}

    def weighted_subtree(self, x, seed_tensor, seeds, topk, gate_ge0=True, do_max_subtree=False, output='saliency', sweep_batch=None,
                         order='numpy', want_top=True):
        """weighted_subtree_ebp of N probes in one engine call (xfr_weighted_subtree_ebp, include/xfr_amd.h).  seeds: 3 x N x D (gate
        output, non-mate output, EBP channel).  output: 'mwp', 'saliency' (ebp_version 6), 'uint8' (the levels, as floats) or 'uint8_saliency'
        (the saliency conversion of ebp_version != 6 of the merged and the top-k maps, levels as floats).
        order: 'numpy' -- np.argsort(w.astype(np.float64)), the reference's own call, through a callback; 'engine' -- the engine's rule
        (stable: ties ascend by firing index); or a callable f(w, probe) -> ascending order of the n_firings float32 weights w.
        Returns (smap N x H1 x W1, top N x topk x H1 x W1 or None -- both device tensors, slots in ascending weight order --, w_valid
        N x topk float32, k_valid N x topk int32 (padding -1), n_valid N int32)."""
        x, _ = self._prep(x)
        n = x.shape[0]
        seeds = seeds.detach().to(self.device, torch.float32).contiguous()
        d = int(np.prod(self.tensor_shape(seed_tensor)))
        if seeds.dim() != 3 or tuple(seeds.shape) != (3, n, d):
            raise ValueError('seeds must be 3 x %d x %d, got %s' % (n, d, tuple(seeds.shape)))
        topk = int(topk)
        c1, h1, w1 = self.tensor_shape(1)
        smap = torch.empty((n, h1, w1), device=self.device)
        top = torch.empty((n, max(topk, 0), h1, w1), device=self.device) if want_top else None
        w_valid = np.zeros((n, max(topk, 0)), dtype=np.float32)
        k_valid = np.full((n, max(topk, 0)), -1, dtype=np.int32)
        n_valid = np.zeros(n, dtype=np.int32)
        if order == 'engine':
            fn = _lib.SUBTREE_ORDER_FN()
        else:
            if order == 'numpy':
                py = lambda w, b: np.argsort(w.astype(np.float64))              # noqa: E731  (whitebox.py:697 on a list of Python floats)
            elif callable(order):
                py = order
            else:
                raise ValueError("order must be 'numpy', 'engine' or a callable, got %r" % (order,))

            def cb(w_ptr, nf, probe, out_ptr, user):
                try:
                    o = np.asarray(py(np.ctypeslib.as_array(w_ptr, shape=(nf,)).copy(), int(probe)), dtype=np.int64)
                    if o.shape != (nf,):
                        return 1
                    np.ctypeslib.as_array(out_ptr, shape=(nf,))[:] = o
                    return 0
                except Exception:
                    return 1
            fn = _lib.SUBTREE_ORDER_FN(cb)          # referenced until the call returns
        args = _lib.SubtreeArgs(topk, 1 if gate_ge0 else 0, 1 if do_max_subtree else 0, self.SUBTREE_OUTPUTS[output], int(sweep_batch or 0),
                                fn, None)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.xfr_weighted_subtree_ebp(self._h, x.data_ptr(), n, int(seed_tensor), seeds.data_ptr(), ctypes.byref(args),
                                                         smap.data_ptr(), top.data_ptr() if top is not None else None,
                                                         w_valid.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                                         k_valid.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                                         n_valid.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), _stream_ptr(self.device)))
        return smap, top, w_valid, k_valid, n_valid

    def ebp_firing(self, x, seed_tensor, seed, firing):
        """Whitebox.P[firing] of a standard sweep: N x C x H x W."""
        x, _ = self._prep(x)
        n = x.shape[0]
        seed = seed.detach().to(self.device, torch.float32).contiguous()
        c, h, w = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.xfr_ebp_store_firing(self._h, x.data_ptr(), n, int(seed_tensor), seed.data_ptr(), int(firing), None,
                                                     ctypes.byref(c), ctypes.byref(h), ctypes.byref(w), _stream_ptr(self.device)))
            out = torch.empty((n, c.value, h.value, w.value), device=self.device)
            _lib.check(self.lib.xfr_ebp_store_firing(self._h, x.data_ptr(), n, int(seed_tensor), seed.data_ptr(), int(firing),
                                                     out.data_ptr(), None, None, None, _stream_ptr(self.device)))
        return out

    # -- STRise blackbox saliency (include/xfr_amd.h: xfr_strise_*) ---------------------------------------
    @staticmethod
    def _strise_tables(cells, shifts, grid, mask_scale):
        """-> (cells int32 n x E, shifts int32 n x 2, StriseGeometry, their ctypes pointers)."""
        cells = np.ascontiguousarray(np.asarray(cells, dtype=np.int32))
        shifts = np.ascontiguousarray(np.asarray(shifts, dtype=np.int32))
        if cells.ndim != 2 or shifts.shape != (cells.shape[0], 2):
            raise ValueError('cells must be n_masks x num_elements and shifts n_masks x 2, got %s and %s' % (cells.shape, shifts.shape))
        geom = _lib.StriseGeometry(int(grid[0]), int(grid[1]), int(mask_scale), int(cells.shape[1]))
        ip = ctypes.POINTER(ctypes.c_int32)
        return cells, shifts, geom, cells.ctypes.data_as(ip), shifts.ctypes.data_as(ip)

    def _strise_options(self, probe_shape, quantize, tables):
        """-> (pointer to an xfr_strise_options or None, (H, W) of the probe, what the pointer refers to).  All three at their defaults: the calls
        as they were (the engine's input size, the closed-form mask law, no quantisation).  tables: (row table, column table) of
        xfr_amd.models.blackbox.pil_bilinear_tables, for luminance engines under quantize."""
        c, h, w = self.program.in_shape
        if probe_shape is None and not quantize and tables is None:
            return None, (h, w), None
        if probe_shape is not None:
            h, w = int(probe_shape[0]), int(probe_shape[1])
        opt = _lib.StriseOptions(struct_size=ctypes.sizeof(_lib.StriseOptions), probe_h=h, probe_w=w, quantize=int(quantize))
        keep = [opt]
        if tables is not None:
            for name, tab in zip(('row_tab', 'col_tab'), tables):
                arr = _tap_array(tab)
                setattr(opt, name, arr)
                keep.append(arr)
        return ctypes.byref(opt), (h, w), keep

    @staticmethod
    def _strise_images(probe_u8, fill, hw, device):
        h, w = hw
        probe_u8 = torch.as_tensor(probe_u8)
        fill = torch.as_tensor(fill)
        if probe_u8.dtype != torch.uint8 or tuple(probe_u8.shape) != (h, w, 3) or tuple(fill.shape) != (h, w, 3):
            raise ValueError('expected a uint8 probe and a fill image of %d x %d x 3, got %s %s and %s' % (h, w, probe_u8.dtype, tuple(probe_u8.shape),
                                                                                                      tuple(fill.shape)))
        return probe_u8.to(device).contiguous(), fill.to(device, torch.float64).contiguous()

    def _strise_open(self, cells, shifts, grid, mask_scale, probe_shape=None, quantize=False, tables=None, first=0, count=None):
        """What the STRise methods open with.  -> (n_masks, the four table arguments of the C calls, the options pointer or None, (H, W) of the probe,
        count with its default: the masks from `first` on, what the pointers refer to)."""
        cells, shifts, geom, cp, sp = self._strise_tables(cells, shifts, grid, mask_scale)
        opt, hw, keep = self._strise_options(probe_shape, quantize, tables)
        n = cells.shape[0]
        return n, (cp, sp, n, ctypes.byref(geom)), opt, hw, n - first if count is None else int(count), (cells, shifts, geom, keep)

    def _call(self, fn, *args):
        """One C call on this engine's device and the current stream."""
        with torch.cuda.device(self.device):
            _lib.check(fn(self._h, *(args + (_stream_ptr(self.device),))))

    def strise_score(self, probe_u8, fill, cells, shifts, grid, mask_scale, refs, gallery, encode_tensor, probe_shape=None, quantize=False, tables=None):
        """The whole STRise sweep of one probe (xfr_strise_score_ex): probe uint8 H x W x 3, fill float64 H x W x 3, refs / gallery fp32 embeddings
        (n x D).  -> (scores float64 [n_masks], orig float64 [n_refs + n_gal]: the unmasked probe's similarities), device tensors.
        quantize: the generator's chain, every masked probe through the uint8 of Whitebox.convert_from_numpy and the engine's own preprocessing."""
        n, tab, opt, hw, _, keep = self._strise_open(cells, shifts, grid, mask_scale, probe_shape, quantize, tables)
        probe_u8, fill = self._strise_images(probe_u8, fill, hw, self.device)
        d = int(np.prod(self.tensor_shape(encode_tensor)))
        refs = refs.detach().to(self.device, torch.float32).reshape(-1, d).contiguous()
        gallery = gallery.detach().to(self.device, torch.float32).reshape(-1, d).contiguous()
        scores = torch.empty(n, device=self.device, dtype=torch.float64)
        orig = torch.empty(refs.shape[0] + gallery.shape[0], device=self.device, dtype=torch.float64)
        self._call(self.lib.xfr_strise_score_ex, probe_u8.data_ptr(), fill.data_ptr(), *(tab + (refs.data_ptr(), refs.shape[0], gallery.data_ptr(),
                   gallery.shape[0], int(encode_tensor), scores.data_ptr(), orig.data_ptr(), opt)))
        return scores, orig

    def strise_combine(self, weights, n_selected, cells, shifts, grid, mask_scale, sign=1, probe_shape=None):
        """xfr_strise_combine_ex: weights float64 [n_masks] (0 for unselected masks) -> the normalised H x W float64 map (device tensor)."""
        n, tab, opt, hw, _, keep = self._strise_open(cells, shifts, grid, mask_scale, probe_shape)
        weights = torch.as_tensor(weights).detach().to(self.device, torch.float64).contiguous()
        if tuple(weights.shape) != (n,):
            raise ValueError('weights must hold %d values, got %s' % (n, tuple(weights.shape)))
        sal = torch.empty(hw, device=self.device, dtype=torch.float64)
        self._call(self.lib.xfr_strise_combine_ex, weights.data_ptr(), int(n_selected), *(tab + (int(sign), sal.data_ptr(), opt)))
        return sal

    def strise_masks(self, cells, shifts, grid, mask_scale, first=0, count=None, probe_shape=None, exact=False):
        """Parity hook: masks [first, first + count) as float64 count x H x W (device tensor); exact: scipy's zoom to the bit
        (xfr_amd.models.blackbox.mask_law_scipy) instead of the closed form (mask_law)."""
        n, tab, opt, hw, count, keep = self._strise_open(cells, shifts, grid, mask_scale, probe_shape, first=first, count=count)
        out = torch.empty((max(count, 0),) + hw, device=self.device, dtype=torch.float64)
        self._call(self.lib.xfr_strise_debug_masks_ex, *(tab + (int(first), count, int(bool(exact)), out.data_ptr(), opt)))
        return out

    def strise_masked_probes(self, probe_u8, fill, cells, shifts, grid, mask_scale, first=0, count=None, probe_shape=None, quantize=False, tables=None):
        """Parity hook: the fp32 network input (count x in_c x in_h x in_w) of masks [first, first + count), count <= max_batch.  With options,
        first = -1 starts at image zero of the sweep, the unmasked probe."""
        n, tab, opt, hw, count, keep = self._strise_open(cells, shifts, grid, mask_scale, probe_shape, quantize, tables, first, count)
        probe_u8, fill = self._strise_images(probe_u8, fill, hw, self.device)
        c, h, w = self.program.in_shape
        out = torch.empty((max(count, 0), c if opt is not None else 3, h, w), device=self.device, dtype=torch.float32)
        self._call(self.lib.xfr_strise_debug_masked_probes_ex, probe_u8.data_ptr(), fill.data_ptr(), *(tab + (int(first), count, out.data_ptr(), opt)))
        return out

    def strise_quantized(self, probe_u8, fill, cells, shifts, grid, mask_scale, first=0, count=None, probe_shape=None):
        """Parity hook (xfr_strise_debug_quantized): q = uint8((v / 255) * 255) of masks [first, first + count), count x H x W x 3 uint8; first = -1
        starts at image zero of the sweep (q = probe)."""
        probe_shape = self.program.in_shape[1:] if probe_shape is None else probe_shape
        n, tab, opt, hw, count, keep = self._strise_open(cells, shifts, grid, mask_scale, probe_shape, True, None, first, count)
        probe_u8, fill = self._strise_images(probe_u8, fill, hw, self.device)
        out = torch.empty((max(count, 0), hw[0], hw[1], 3), device=self.device, dtype=torch.uint8)
        self._call(self.lib.xfr_strise_debug_quantized, probe_u8.data_ptr(), fill.data_ptr(), *(tab + (int(first), count, out.data_ptr(), opt)))
        return out

    # -- inpainting-game scoring (include/xfr_amd.h: xfr_inpaint_*) -----------------------------------------
    def _inpaint_masks_args(self, sal, noise, levels, method, size=None):
        """-> (sal float64 n_maps x H x W on the device, noise or None, levels float64 host array, its ctypes pointer, method id)."""
        sal = torch.as_tensor(sal)
        if sal.dim() == 2:
            sal = sal.unsqueeze(0)
        c, h, w = self.program.in_shape
        if sal.dim() != 3 or (size is None and tuple(sal.shape[1:]) != (h, w)):
            raise ValueError('expected saliency maps n_maps x %d x %d (the engine input size), got %s' % (h, w, tuple(sal.shape)))
        sal = sal.detach().to(self.device, torch.float64).contiguous()
        if noise is not None:
            noise = torch.as_tensor(noise)
            if tuple(noise.shape) != tuple(sal.shape[1:]):
                raise ValueError('expected noise of %s, got %s' % (tuple(sal.shape[1:]), tuple(noise.shape)))
            noise = noise.detach().to(self.device, torch.float64).contiguous()
        levels = np.ascontiguousarray(np.asarray(levels, dtype=np.float64).ravel())
        if method not in (_lib.INPAINT_PERCENT_DENSITY, _lib.INPAINT_THRESHOLDS):
            method = {'percent-density': _lib.INPAINT_PERCENT_DENSITY, 'thresholds': _lib.INPAINT_THRESHOLDS}.get(method, -1 if isinstance(method, str) else method)
        return sal, noise, levels, levels.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), int(method)

    def _inpaint_options(self, n_maps, levels, totals=None, levels_per_map=False, blur_kernel=None, blur_levels=None):
        """-> (xfr_inpaint_options by reference or None when every option is at its default, n_levels, the host arrays it points to).
        totals: n_maps sums, the caller's own (s = v / total); levels_per_map: `levels` is n_maps x n_levels; blur_kernel: the 2 r + 1 weights of
        inpainting_score.gaussian_kernel1d; blur_levels: n_levels flags, False leaves a level hard."""
        n_levels = len(levels)
        if levels_per_map:
            if n_maps < 1 or len(levels) % n_maps:
                raise ValueError('expected %d rows of levels, got %d values' % (n_maps, len(levels)))
            n_levels = len(levels) // n_maps
        if totals is None and not levels_per_map and blur_kernel is None and blur_levels is None:
            return None, n_levels, ()
        opt = _lib.InpaintOptions()
        opt.struct_size = ctypes.sizeof(_lib.InpaintOptions)
        opt.levels_per_map = 1 if levels_per_map else 0
        keep = []
        if totals is not None:
            t = np.ascontiguousarray(np.asarray(totals, dtype=np.float64).ravel())
            if t.size != n_maps:
                raise ValueError('expected %d totals, got %d' % (n_maps, t.size))
            opt.totals_host = t.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
            keep.append(t)
        if blur_kernel is not None:
            k = np.ascontiguousarray(np.asarray(blur_kernel, dtype=np.float64).ravel())
            if k.size % 2 != 1:
                raise ValueError('expected a blur kernel of 2 r + 1 weights, got %d' % k.size)
            opt.blur_radius = k.size // 2
            opt.blur_kernel_host = k.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
            keep.append(k)
        if blur_levels is not None:
            f = np.ascontiguousarray(np.asarray(blur_levels).ravel() != 0).astype(np.uint8)
            if f.size != n_levels:
                raise ValueError('expected %d blur flags, got %d' % (n_levels, f.size))
            opt.blur_level_host = f.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
            keep.append(f)
        return ctypes.byref(opt), n_levels, (opt, keep)

    def _inpaint_images(self, orig, inpaint):
        shape = tuple(self.program.in_shape)
        orig, inpaint = torch.as_tensor(orig), torch.as_tensor(inpaint)
        if tuple(orig.shape) != shape or tuple(inpaint.shape) != shape:
            raise ValueError('expected the original and its inpainted twin in network format %s, got %s and %s' % (shape, tuple(orig.shape), tuple(inpaint.shape)))
        return orig.detach().to(self.device, torch.float32).contiguous(), inpaint.detach().to(self.device, torch.float32).contiguous()

    def _inpaint_call(self, name, mask_args, tail, opt):
        """xfr_inpaint_<name> when opt is None, else xfr_inpaint_<name>_ex with opt behind the tail.  mask_args: (sal, noise, max_noise, include_zero,
        method id, levels pointer, n_levels) -- the leading arguments of every entry point, and (h, w) of the maps behind them where the entry point
        takes them behind n_maps; tail: its own arguments."""
        sal, noise, max_noise, include_zero, method, lp, n_levels = mask_args[:7]
        args = (sal.data_ptr(), sal.shape[0]) + tuple(mask_args[7:]) + (noise.data_ptr() if noise is not None else None, float(max_noise),
                                                                        1 if include_zero else 0, method, lp, n_levels) + tuple(tail)
        if opt is None:
            self._call(getattr(self.lib, 'xfr_inpaint_' + name), *args)
        else:
            self._call(getattr(self.lib, 'xfr_inpaint_%s_ex' % name), *(args + (opt,)))

    def inpaint_score(self, sal, levels, orig, inpaint, gal_orig, gal_inp, encode_tensor, method='percent-density', noise=None, max_noise=1e-9,
                      include_zero=True, totals=None, levels_per_map=False, blur_kernel=None, blur_levels=None):
        """xfr_inpaint_score: the inpainting game of n_maps maps of one probe.  sal n_maps x H x W float64, levels percentiles (or thresholds), orig /
        inpaint in_c x H x W fp32 network tensors, gal_orig / gal_inp D-vectors.  -> (cls uint8, pg float64, pr float64), n_maps x n_levels device tensors.
        totals, levels_per_map, blur_kernel, blur_levels: xfr_inpaint_options (_inpaint_options); any of them set calls xfr_inpaint_score_ex."""
        sal, noise, levels, lp, method = self._inpaint_masks_args(sal, noise, levels, method)
        opt, n_levels, keep = self._inpaint_options(sal.shape[0], levels, totals, levels_per_map, blur_kernel, blur_levels)
        orig, inpaint = self._inpaint_images(orig, inpaint)
        try:
            d = int(np.prod(self.tensor_shape(encode_tensor)))
        except ValueError:
            d = None          # xfr_inpaint_score refuses the tensor id itself, naming it
        gals = [torch.as_tensor(g).detach().to(self.device, torch.float32).reshape(-1).contiguous() for g in (gal_orig, gal_inp)]
        if d is not None and (gals[0].numel() != d or gals[1].numel() != d):
            raise ValueError('expected gallery embeddings of %d values, got %d and %d' % (d, gals[0].numel(), gals[1].numel()))
        shape = (sal.shape[0], max(n_levels, 1))
        pg = torch.empty(shape, device=self.device, dtype=torch.float64)
        pr = torch.empty(shape, device=self.device, dtype=torch.float64)
        cls = torch.empty(shape, device=self.device, dtype=torch.uint8)
        self._inpaint_call('score', (sal, noise, max_noise, include_zero, method, lp, n_levels),
                           (orig.data_ptr(), inpaint.data_ptr(), gals[0].data_ptr(), gals[1].data_ptr(), int(encode_tensor), pg.data_ptr(), pr.data_ptr(),
                            cls.data_ptr()), opt)
        return cls, pg, pr

    def inpaint_iou(self, sal, levels, ground_truth, method='percent-density', noise=None, max_noise=1e-9, include_zero=True, totals=None,
                    levels_per_map=False, **blur):
        """xfr_inpaint_iou: -> int64 n_maps x n_levels x 3 (device tensor): |gt & mask|, |gt | mask|, |~gt & mask|.  totals, levels_per_map:
        xfr_inpaint_iou_ex (which refuses a blur: the counts are of hard masks)."""
        sal, noise, levels, lp, method = self._inpaint_masks_args(sal, noise, levels, method)
        opt, n_levels, keep = self._inpaint_options(sal.shape[0], levels, totals, levels_per_map, **blur)
        gt = torch.as_tensor(ground_truth)
        if tuple(gt.shape) != tuple(sal.shape[1:]):
            raise ValueError('expected a ground truth of %s, got %s' % (tuple(sal.shape[1:]), tuple(gt.shape)))
        gt = (gt != 0).to(self.device, torch.uint8).contiguous()
        counts = torch.empty((sal.shape[0], max(n_levels, 1), 3), device=self.device, dtype=torch.int64)
        self._inpaint_call('iou', (sal, noise, max_noise, include_zero, method, lp, n_levels), (gt.data_ptr(), counts.data_ptr()), opt)
        return counts

    def inpaint_masks(self, sal, levels, method='percent-density', noise=None, max_noise=1e-9, include_zero=True, want_cdf=False, totals=None,
                      levels_per_map=False, **blur):
        """Parity hook (xfr_inpaint_debug_masks), maps of any size: -> first_on uint8 n_maps x h x w (mask l is first_on <= l), and with want_cdf the
        float64 value every pixel was compared by.  totals, levels_per_map: xfr_inpaint_debug_masks_ex."""
        sal, noise, levels, lp, method = self._inpaint_masks_args(sal, noise, levels, method, size='any')
        opt, n_levels, keep = self._inpaint_options(sal.shape[0], levels, totals, levels_per_map, **blur)
        first_on = torch.empty(tuple(sal.shape), device=self.device, dtype=torch.uint8)
        cdf = torch.empty(tuple(sal.shape), device=self.device, dtype=torch.float64) if want_cdf else None
        self._inpaint_call('debug_masks', (sal, noise, max_noise, include_zero, method, lp, n_levels, sal.shape[1], sal.shape[2]),
                           (first_on.data_ptr(), cdf.data_ptr() if want_cdf else None), opt)
        return (first_on, cdf) if want_cdf else first_on

    def inpaint_soft_masks(self, sal, levels, method='percent-density', noise=None, max_noise=1e-9, include_zero=True, totals=None, levels_per_map=False,
                           blur_kernel=None, blur_levels=None, first=0, count=None):
        """Parity hook (xfr_inpaint_debug_soft_masks), maps of any size: the float64 masks [first, first + count) of the n_maps * n_levels list as the
        hybrids see them, count x h x w; without a blur kernel the hard masks as 0.0 / 1.0."""
        sal, noise, levels, lp, method = self._inpaint_masks_args(sal, noise, levels, method, size='any')
        opt, n_levels, keep = self._inpaint_options(sal.shape[0], levels, totals, levels_per_map, blur_kernel, blur_levels)
        count = sal.shape[0] * n_levels - first if count is None else int(count)
        out = torch.empty((max(count, 0),) + tuple(sal.shape[1:]), device=self.device, dtype=torch.float64)
        # one entry point, with the options in the middle of its own arguments
        self._inpaint_call('debug_soft_masks', (sal, noise, max_noise, include_zero, method, lp, n_levels),
                           (sal.shape[1], sal.shape[2], opt, int(first), count, out.data_ptr()), None)
        return out

    def inpaint_blends(self, sal, levels, orig, inpaint, method='percent-density', noise=None, max_noise=1e-9, include_zero=True, first=0, count=None,
                       totals=None, levels_per_map=False, blur_kernel=None, blur_levels=None):
        """Parity hook (xfr_inpaint_debug_blends): the fp32 hybrids [first, first + count) of the n_maps * n_levels list, count x in_c x H x W.
        totals, levels_per_map, blur_kernel, blur_levels: xfr_inpaint_debug_blends_ex."""
        sal, noise, levels, lp, method = self._inpaint_masks_args(sal, noise, levels, method)
        opt, n_levels, keep = self._inpaint_options(sal.shape[0], levels, totals, levels_per_map, blur_kernel, blur_levels)
        orig, inpaint = self._inpaint_images(orig, inpaint)
        count = sal.shape[0] * n_levels - first if count is None else int(count)
        out = torch.empty((max(count, 0),) + tuple(self.program.in_shape), device=self.device, dtype=torch.float32)
        self._inpaint_call('debug_blends', (sal, noise, max_noise, include_zero, method, lp, n_levels),
                           (orig.data_ptr(), inpaint.data_ptr(), int(first), count, out.data_ptr()), opt)
        return out

    # -- match calibration (include/xfr_amd.h: xfr_embed_templates, xfr_pair_dists, xfr_nearest_rows) ------------------
    def _matrix(self, x, what):
        x = torch.as_tensor(x)
        if x.dim() != 2:
            raise ValueError('expected %s as a matrix of rows, got %s' % (what, tuple(x.shape)))
        return x.detach().to(self.device, torch.float32).contiguous()

    @staticmethod
    def _int_table(values, shape=None):
        t = np.ascontiguousarray(np.asarray(values, dtype=np.int64))
        if shape is not None:
            t = t.reshape(shape)
        if t.size and (t.min() < -2 ** 31 or t.max() >= 2 ** 31):
            raise ValueError('an index table holds int32 values')
        t = np.ascontiguousarray(t.astype(np.int32))
        return t, t.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))

    def embed_templates(self, emb, rows, offsets, normalize_rows=True):
        """xfr_embed_templates: emb n x D fp32, rows a list of row indices (repeats allowed), offsets G + 1 places in it.
        -> G x D fp32 templates (device tensor): the group's rows, each divided by its norm first with normalize_rows, averaged (summed without) and
        divided by the norm of the result."""
        emb = self._matrix(emb, 'the embeddings')
        rows, rp = self._int_table(rows, (-1,))
        offsets, op = self._int_table(offsets, (-1,))
        if offsets.size < 2 or offsets[-1] != rows.size:
            raise ValueError('expected offsets from 0 to the %d rows of the list, got %s' % (rows.size, offsets.tolist()[:8]))
        out = torch.empty((offsets.size - 1, emb.shape[1]), device=self.device, dtype=torch.float32)
        self._call(self.lib.xfr_embed_templates, emb.data_ptr(), emb.shape[0], emb.shape[1], rp, op, offsets.size - 1, 1 if normalize_rows else 0,
                   out.data_ptr())
        return out

    def pair_dists(self, a, b, pairs):
        """xfr_pair_dists: a na x D, b nb x D fp32, pairs np x 2 row indices (i into a, j into b) -> |a[i] - b[j]| fp32 [np] (device tensor)."""
        a, b = self._matrix(a, 'A'), self._matrix(b, 'B')
        if a.shape[1] != b.shape[1]:
            raise ValueError('rows of %d and of %d values' % (a.shape[1], b.shape[1]))
        pairs, pp = self._int_table(pairs, (-1, 2))
        out = torch.empty(pairs.shape[0], device=self.device, dtype=torch.float32)
        self._call(self.lib.xfr_pair_dists, a.data_ptr(), a.shape[0], b.data_ptr(), b.shape[0], a.shape[1], pp, pairs.shape[0], out.data_ptr())
        return out

    def nearest_rows(self, queries, gallery, k, exclude_same_index=False):
        """xfr_nearest_rows: the k nearest gallery rows of every query -> (idx int32, dist fp32), nq x k device tensors, in increasing distance,
        equal distances by lower index; exclude_same_index: query i ignores gallery row i."""
        q, g = self._matrix(queries, 'the queries'), self._matrix(gallery, 'the gallery')
        if q.shape[1] != g.shape[1]:
            raise ValueError('rows of %d and of %d values' % (q.shape[1], g.shape[1]))
        k = int(k)
        idx = torch.empty((q.shape[0], max(k, 0)), device=self.device, dtype=torch.int32)
        dist = torch.empty((q.shape[0], max(k, 0)), device=self.device, dtype=torch.float32)
        self._call(self.lib.xfr_nearest_rows, q.data_ptr(), q.shape[0], g.data_ptr(), g.shape[0], q.shape[1], k, 1 if exclude_same_index else 0,
                   idx.data_ptr(), dist.data_ptr())
        return idx, dist

    # -- saliency finishing (include/xfr_amd.h: xfr_finish_saliency) ---------------------------------------------
    def _finish_call(self, *args):
        """xfr_finish_saliency on this engine's device and the current stream; a refused call raises XfrError with the library's text."""
        with torch.cuda.device(self.device):
            status = self.lib.xfr_finish_saliency(self._h, *(args + (_stream_ptr(self.device),)))
        if status != _lib.XFR_OK:
            raise _lib.XfrError(status, self.lib.xfr_last_error().decode('utf-8', 'replace'))

    def finish_saliency(self, maps, out_hw, probes_u8=None, totals=None):
        """xfr_finish_saliency: create_save_smap's arithmetic for n maps at once.  maps float32 n x h x w (host or device), out_hw the probes' (H, W),
        probes_u8 uint8 n x H x W x 3 or None, totals n float32 sums of the shifted maps or None (the device's own: the float32 nearest to the sum).
        -> (sal float64 n x H x W, overlay uint8 n x H x W x 3 or None), device tensors."""
        from .saliency_io import jet
        maps = torch.as_tensor(maps)
        if maps.dim() == 2:
            maps = maps.unsqueeze(0)
        if maps.dim() != 3 or maps.dtype != torch.float32:
            raise ValueError('expected float32 maps n x h x w, got %s of %s' % (maps.dtype, tuple(maps.shape)))
        maps = maps.detach().to(self.device).contiguous()
        n, (H, W) = maps.shape[0], (int(out_hw[0]), int(out_hw[1]))
        tp = None
        if totals is not None:
            totals = np.ascontiguousarray(np.asarray(totals, dtype=np.float32).ravel())
            if totals.size != n:
                raise ValueError('expected %d totals, got %d' % (n, totals.size))
            tp = totals.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        sal = torch.empty((n, H, W), device=self.device, dtype=torch.float64)
        probes = overlay = lut = lp = None
        if probes_u8 is not None:
            probes = torch.as_tensor(probes_u8)
            if probes.dtype != torch.uint8 or tuple(probes.shape) != (n, H, W, 3):
                raise ValueError('expected uint8 probes %s, got %s of %s' % ((n, H, W, 3), probes.dtype, tuple(probes.shape)))
            probes = probes.detach().to(self.device).contiguous()
            overlay = torch.empty((n, H, W, 3), device=self.device, dtype=torch.uint8)
            lut = np.ascontiguousarray(jet(np.arange(256) / 256.0), dtype=np.float64)      # saliency_io's own table, row by row
            lp = lut.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        self._finish_call(maps.data_ptr(), n, maps.shape[1], maps.shape[2], H, W, tp, probes.data_ptr() if probes is not None else None, lp,
                          sal.data_ptr(), overlay.data_ptr() if overlay is not None else None)
        return sal, overlay

    # -- image intake (include/xfr_amd.h: xfr_intake_u8, xfr_intake_u8_host, xfr_intake_set_kernels) ---------------
    def intake_set_kernels(self, sigmas, radii, weights):
        """xfr_intake_set_kernels: the caller's Gaussian kernels for the pre-filter (xfr_amd.intake.stated_kernels: numpy's), replacing those stated
        before.  weights: n x (INTAKE_MAX_RADIUS + 1), row i the normalised weights of x = -radii[i] .. 0."""
        sigmas = np.ascontiguousarray(sigmas, dtype=np.float64).ravel()
        radii = np.ascontiguousarray(radii, dtype=np.int32).ravel()
        weights = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1, _lib.INTAKE_MAX_RADIUS + 1)
        if not (sigmas.size == radii.size == weights.shape[0]):
            raise ValueError('expected as many sigmas, radii and rows of weights, got %d, %d and %d' % (sigmas.size, radii.size, weights.shape[0]))
        dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
        _lib.check(self.lib.xfr_intake_set_kernels(self._h, sigmas.ctypes.data_as(dp), radii.ctypes.data_as(ip), weights.ctypes.data_as(dp), sigmas.size))

    def intake_u8(self, src, items, out_hw, tables=None):
        """xfr_intake_u8 (src a uint8 device tensor) or xfr_intake_u8_host (src a uint8 numpy array or host tensor): the crops `items` (an array of
        xfr_amd.intake.Item inside src) resized to out_hw as convert_from_numpy does it, then, with tables = (row, column) of pil_bilinear_tables,
        through Pillow's integer resize and crop.  -> uint8 device tensor n x H x W x 3 (n x len(row) x len(column) x 3 with tables).  A refused
        call raises XfrError with the library's text."""
        n = len(items)
        H, W = int(out_hw[0]), int(out_hw[1])
        row = col = None
        fh, fw = H, W
        if tables is not None:
            row, col = _tap_array(tables[0]), _tap_array(tables[1])
            fh, fw = len(row), len(col)
        on_device = isinstance(src, torch.Tensor) and src.is_cuda
        if on_device:
            if src.dtype != torch.uint8:
                raise ValueError('expected a uint8 source, got %s' % src.dtype)
            src = src.detach().to(self.device).contiguous()
            ptr, nbytes, fn = src.data_ptr(), src.numel(), self.lib.xfr_intake_u8
        else:
            src = np.ascontiguousarray(src.numpy() if isinstance(src, torch.Tensor) else src)
            if src.dtype != np.uint8:
                raise ValueError('expected a uint8 source, got %s' % src.dtype)
            ptr, nbytes, fn = src.ctypes.data, src.size, self.lib.xfr_intake_u8_host
        out = torch.empty((max(n, 0), fh, fw, 3), device=self.device, dtype=torch.uint8)
        with torch.cuda.device(self.device):
            status = fn(self._h, ptr, nbytes, ctypes.cast(items, ctypes.c_void_p), n, H, W, row, col, fh, fw, out.data_ptr(), _stream_ptr(self.device))
        if status != _lib.XFR_OK:
            raise _lib.XfrError(status, self.lib.xfr_last_error().decode('utf-8', 'replace'))
        return out

    # ------------------------------------------------------------------------------------------------
    def set_trace(self, on):
        _lib.check(self.lib.xfr_engine_set_trace(self._h, 1 if on else 0))

    def get_trace(self):
        """(sums [n_firings, S*N] float64, names [n_firings]) of the last ebp call, reference firing order."""
        nf = ctypes.c_int32()
        _lib.check(self.lib.xfr_engine_trace_size(self._h, ctypes.byref(nf)))
        cap = nf.value * 2 * self.max_batch
        sums = (ctypes.c_double * max(cap, 1))()
        kinds = (ctypes.c_int32 * max(nf.value, 1))()
        _lib.check(self.lib.xfr_engine_get_trace(self._h, sums, kinds, cap))
        arr = np.frombuffer(sums, dtype=np.float64)
        names = [LAYER_NAMES[OpKind(k)] for k in list(kinds)[:nf.value]]
        return arr, names, nf.value

    def set_profile(self, on):
        _lib.check(self.lib.xfr_engine_set_profile(self._h, 1 if on else 0))

    def profile_csv(self, path):
        """Append one CSV record per GEMM launch to `path` while profiling is on (None: stop)."""
        _lib.check(self.lib.xfr_engine_profile_csv(self._h, path.encode() if path else None))

    def get_profile_by_kernel(self):
        """The last profiled run's GEMM launches by the kernel family that ran them: {'fp32': (ms, launches, flops), 'bf16x6': (...)}."""
        ms, n, fl = (ctypes.c_double * 2)(), (ctypes.c_int64 * 2)(), (ctypes.c_double * 2)()
        _lib.check(self.lib.xfr_engine_get_profile_by_kernel(self._h, ms, n, fl))
        return {'fp32': (ms[0], n[0], fl[0]), 'bf16x6': (ms[1], n[1], fl[1])}

    def get_profile(self):
        ms, n, fl = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
        _lib.check(self.lib.xfr_engine_get_profile(self._h, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl)))
        return ms.value, n.value, fl.value

