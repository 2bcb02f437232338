"""Inputs of the soft-mask / percent-pixels fixture (tests/golden/golden_inpaint_soft.npz), shared by its generator and the tests that replay it.
Probes, twins, gallery pairs and maps are those of inpaint_game_inputs (seeded functions of the case), so the fixture stores results only.

A case: (arch, threshold method, levels, include_zero_elements, maps in the call, mask_blur_sigma in percent of min(H, W) or None)."""
import numpy as np

import inpaint_game_inputs as I

STANDARD, COARSE = I.STANDARD, I.COARSE

CASES = {
    'mini/blur4': ('stresnet_mini', 'percent-density', STANDARD, True, 1, 4),
    'mini/blur1': ('stresnet_mini', 'percent-density', STANDARD, True, 1, 1),                   # radius 9: smaller than any tile
    'mini/blur4_zero_off': ('stresnet_mini', 'percent-density', STANDARD, False, 1, 4),
    'mini/pixels': ('stresnet_mini', 'percent-pixels', STANDARD, True, 1, None),
    'mini/pixels_blur4': ('stresnet_mini', 'percent-pixels', STANDARD, True, 1, 4),
    'mini/two_maps_pixels': ('stresnet_mini', 'percent-pixels', STANDARD, True, 2, None),       # the thresholds differ per map
    'lcnn/blur4': ('lightcnn29v2', 'percent-density', STANDARD, True, 1, 4),                    # one channel, 128 x 128, radius 20
    'r101/coarse_blur4': ('stresnet101', 'percent-density', COARSE, True, 1, 4),
}


def maps_of(name, seed):
    arch, _, _, _, n_maps, _ = CASES[name]
    return np.stack([I.bump_map(I.in_shape(arch)[1:], seed + 1000 * k) for k in range(n_maps)])


def sigma_px(name):
    arch, blur = CASES[name][0], CASES[name][5]
    return None if blur is None else blur * min(I.in_shape(arch)[1:]) / 100.0


def stored_levels(n_levels):
    """The three levels whose blurred masks the fixture keeps rows of."""
    return np.array([n_levels // 10, n_levels // 2, (9 * n_levels) // 10])


def stored_rows(h):
    return np.array([0, h // 2, h - 1])
