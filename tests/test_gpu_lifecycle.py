"""GPU test of the engine's life cycle: every family of entry points once on one engine of the mini ResNet -- so that every lazily built group of
device buffers, pinned buffers, events and streams exists (csrc/hip_owner.h) --, then close(), then the same calls on a second engine built from the
same weights.  Every output of the second pass equals the first byte for byte: nothing of the first engine is needed, and nothing of it is in the way.
(What is freed is counted on the host, tests/test_hip_owner.py: the card's free memory is other work's too.)"""
import numpy as np
import pytest
import torch

import inpaint_game_inputs as G
import intake_inputs as I
from parity_utils import make_backbone, make_images
from xfr_amd import intake, synth
from xfr_amd.engine import Engine
from xfr_amd.models import resnet

pytestmark = pytest.mark.gpu
ARCH, BATCH = 'stresnet_mini', 8


def _every_family_once(prog, sd, device):
    """-> [(name, host array)] of one engine's life: built, every family called once, closed."""
    eng = Engine(prog, BATCH, device)
    eng.load_weights(sd)
    eng.set_mode('affineonly_with_prior')
    eng.set_u8_preprocess('sub_mean', 3, tuple(float(v) for v in resnet.MEAN_RGB), None)
    enc = prog.marks['encode']
    d = int(np.prod(eng.tensor_shape(enc)))
    out = []

    def keep(name, *tensors):
        for k, t in enumerate(tensors):
            out.append(('%s[%d]' % (name, k), t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)))

    x = make_images(ARCH, 4, seed=1)
    pair = torch.stack((synth.unit_rows(4, d, seed=11), synth.unit_rows(4, d, seed=21))) / 2500
    keep('contrastive', eng.contrastive(x, enc, pair))
    eng.set_pipeline(7)                                   # every run call pipelined, three forward slots
    keep('triplet', eng.triplet_contrastive(x, torch.cat((x, x.flip(0)), dim=0), enc))
    g = torch.Generator().manual_seed(11)
    probes_u8 = torch.randint(0, 256, (4, 224, 224, 3), generator=g, dtype=torch.uint8)
    gallery_u8 = torch.randint(0, 256, (8, 224, 224, 3), generator=g, dtype=torch.uint8)
    keep('triplet_u8_host', eng.triplet_contrastive_u8_host(probes_u8, gallery_u8, enc))
    eng.wait_inputs_copied()
    eng.set_pipeline(0)
    # layerwise with one capture: the element of firing 3 that xfr_subtree_weights names, its value as the prior of one sweep
    x1 = x[:1]
    w, idx = eng.subtree_weights(x1, enc, pair[:, :1])
    cap = eng.ebp_capture(x1, enc, pair[:1, :1], idx[:, 0])
    keep('subtree_weights', w, idx)
    keep('capture', cap)
    keep('layerwise', eng.layerwise(x1, enc, [3], [int(idx[3, 0])], [float(cap[3])]))
    seeds = torch.stack([synth.unit_rows(2, d, seed=31 + k) for k in range(3)]) / 2500
    keep('weighted_subtree', *eng.weighted_subtree(x[:2], enc, seeds, 2, order='engine'))
    maps = torch.from_numpy(np.stack([G.bump_map((14, 14), seed=5 + k) for k in range(2)]).astype(np.float32))
    keep('finish', *eng.finish_saliency(maps, (224, 224), probes_u8=probes_u8[:2]))
    crops = [(I.random_image(96, 131, 3, seed=50), I.HEADS[0]), (I.ramp(57, 40, 1), I.HEADS[1])]
    src, table = intake.pack(crops)
    eng.intake_set_kernels(*intake.stated_kernels(crops, (224, 224)))
    keep('intake_host', eng.intake_u8(src, table, (224, 224)))
    a, b = synth.unit_rows(6, 64, seed=41), synth.unit_rows(5, 64, seed=42)
    keep('pair_dists', eng.pair_dists(a, b, [[0, 4], [5, 0], [2, 2]]))
    # 12 masks: two batches of the sweep, the second padded
    rng = np.random.RandomState(7)
    cells = rng.randint(0, 361, size=(12, 1)).astype(np.int32)
    shifts = rng.randint(0, 12, size=(12, 2)).astype(np.int32)
    emb = synth.unit_rows(3, d, seed=43)
    keep('strise', *eng.strise_score(probes_u8[0], torch.full((224, 224, 3), 0.5, dtype=torch.float64), cells, shifts, (19, 19), 12, emb, emb, enc))
    orig, twin = G.probe_pair(ARCH)
    keep('inpaint', *eng.inpaint_score(G.bump_map((224, 224), seed=9)[None], [30.0, 60.0], orig, twin, emb[0], emb[1], enc))
    torch.cuda.synchronize()
    eng.close()
    return out


def test_a_second_engine_repeats_the_first_to_the_byte(gpu_device):
    bb, sd = make_backbone(ARCH, seed=3, num_classes=5)
    prog = bb.build_program()
    first = _every_family_once(prog, sd, gpu_device)
    second = _every_family_once(prog, sd, gpu_device)
    assert [n for n, _ in first] == [n for n, _ in second] and len(first) >= 20
    for (name, u), (_, v) in zip(first, second):
        assert u.shape == v.shape and u.dtype == v.dtype and u.size > 0, name
        assert np.isfinite(u.astype(np.float64)).all(), name
        assert u.tobytes() == v.tobytes(), '%s differs between the two engines' % name
