"""The case table of tests/grouped_direct_cases.py, checked without a device: every case's stated K, M and tile against its shape and against the
restated sizing loop of launch_conv_depthwise, the branches the table claims (VEC or scalar, tiles, row blocks), and -- what makes the table a test of the
launches the engine really makes -- that the backward-role and phase launches, fed through the float64 reference with their prepared weights, are torch
autograd's input gradient of the forward layer to 1e-12 relative."""
import pytest
import torch
import torch.nn.functional as F

import grouped_direct_cases as C


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


def test_names_are_unique_and_every_table_row_is_there():
    assert len(C.BY_NAME) == len(C.CASES)
    want = ['vec_tiles', 'm1024', 'm1025', 'co2', 'co5', 'co8', 'ci8', 'tm512', 'tm512_batch', 'tm256', 'tm256_odd', 'tm128', 'tm128_odd', 'no_tile', 'cap_co9',
            'cap_ci9', 'cap_k8', 'cap_pair', 'gdc', 'k1_s2', 'k1_pad2', 'k7_on_3x2', 'taps_3x5', 'taps_5x3', 'scatter_vec', 'scatter_odd', 'prefix_odd', 'prefix_vec',
            'in_off1', 'out_off1', 'acc_vec', 'rb4/nb2', 'rb4/nb3', 'rb4_ragged/nb2', 'rb4_ragged/nb3', 'rb4_back/nb2', 'rb4_back/nb3', 'rb2_k1/nb2', 'rb2_k1/nb3',
            'm257/nb1']
    assert not [n for n in want if n not in C.BY_NAME]
    assert all(n in C.BY_NAME for n in C.ISOLATION)


@pytest.mark.parametrize('name', [c.name for c in C.CASES])
def test_stated_figures_match_the_shape(name):
    c = C.BY_NAME[name]
    inp = C.inputs(c)
    assert tuple(inp['w'].shape) == (c.G * c.Co, c.Ci, c.kh, c.kw) and tuple(inp['x'].shape) == (c.G * c.Ci, c.in_nb, c.H, c.W)
    assert c.K == c.Ci * c.kh * c.kw and c.M == c.NB * c.OH * c.OW, (c.K, c.Ci * c.kh * c.kw, c.M, c.NB * c.OH * c.OW)
    assert c.OH >= 1 and c.OW >= 1 and c.NB <= c.in_nb and c.NB <= c.out_nb
    (r0, c0), s = c.origin, c.out_stride
    assert (c.OH - 1) * s + r0 < c.target[0] and (c.OW - 1) * s + c0 < c.target[1]
    tm = C.launcher_tile(c)
    if c in C.GROUPED:
        assert c.expect == (C.CFG_GROUP, 0) and c.nhalves == 2 and tm == 0
    else:
        assert c.expect == ((C.CFG_DEPTHWISE, tm) if tm else (C.CFG_GROUP, 0)), (c.expect, tm)
    assert bool(torch.isnan(inp['x'][:, c.NB:]).all()) and bool(torch.isfinite(inp['x'][:, :c.NB]).all())
    r64 = C.reference(c, inp)
    assert all(bool(torch.isfinite(t).all()) for t in r64)
    if c.nhalves == 1:
        assert torch.equal(r64[1], inp['pre1'].double())


def test_the_branches_the_table_claims():
    B = C.BY_NAME
    tiles = lambda c: -(-c.M // c.expect[1])
    vec = lambda c: c.OW % 4 == 0
    assert tiles(B['vec_tiles']) == 2 and vec(B['vec_tiles']) and B['vec_tiles'].W % 4 == 0
    # the border of vec_tiles' two tiles: output 1024 is image 7, row 1, column 4
    assert divmod(1024, 144) == (7, 16) and divmod(16, 12) == (1, 4)
    assert tiles(B['m1024']) == 1 and tiles(B['m1025']) == 2 and not vec(B['m1025'])
    assert [B[n].Co for n in ('co2', 'co5', 'co8')] == [2, 5, 8] and all(B[n].nhalves == 2 and vec(B[n]) for n in ('co2', 'co5', 'co8'))
    assert B['ci8'].Ci == 8 and B['ci8'].Co == 1
    assert tiles(B['tm512']) == 2 and vec(B['tm512']) and tiles(B['tm512_batch']) == 3 and 512 // 9 == 56
    assert tiles(B['tm256']) == 4 and vec(B['tm256']) and not vec(B['tm256_odd']) and B['tm256_odd'].W % 4 != 0
    assert tiles(B['tm128']) == 2 and vec(B['tm128']) and tiles(B['tm128_odd']) == 2 and not vec(B['tm128_odd'])
    assert [B[n].expect[1] for n in ('tm512', 'tm512_batch', 'tm256', 'tm256_odd', 'tm128', 'tm128_odd')] == [512, 512, 256, 256, 128, 128]
    for n in ('no_tile', 'cap_co9', 'cap_ci9', 'cap_k8', 'cap_pair'):
        assert not B[n].eligible
    # no_tile is refused by the budget alone, the caps by the caps alone
    assert max(B['no_tile'].Ci, B['no_tile'].Co) <= C.MAX_CH and B['no_tile'].kh <= C.MAX_TAP and min(B['no_tile'].Ci, B['no_tile'].Co) == 1
    assert B['cap_co9'].Co == 9 and B['cap_ci9'].Ci == 9 and B['cap_k8'].kh == 8 and (B['cap_pair'].Ci, B['cap_pair'].Co) == (2, 2)
    assert (B['gdc'].M, B['gdc'].OW) == (5, 1)
    assert B['k1_s2'].stride > B['k1_s2'].kh and B['k7_on_3x2'].kh > B['k7_on_3x2'].H
    assert B['taps_3x5'].pad_dw > 0 > B['taps_5x3'].pad_dw
    for n, v in (('scatter_vec', True), ('scatter_odd', False), ('phase_vec', True), ('phase_odd', False)):
        c = B[n]
        assert vec(c) == v and c.out_stride == 2 and c.origin == (1, 1) and c.accumulate == 1 and not c.dense
    assert B['scatter_vec'].target == (2 * B['scatter_vec'].OH + 1, 2 * B['scatter_vec'].OW)
    assert B['scatter_odd'].target == (2 * B['scatter_odd'].OH + 1, 2 * B['scatter_odd'].OW)
    assert vec(B['prefix_vec']) and not vec(B['prefix_odd']) and all(B[n].in_nb == 8 and B[n].out_nb == 5 and B[n].NB == 3 for n in ('prefix_vec', 'prefix_odd'))
    assert B['in_off1'].in_shift == 1 and B['out_off1'].out_shift == 1 and B['acc_vec'].accumulate == 1 and B['acc_vec'].nhalves == 2
    # the grouped kernel: row blocks of 16 channels, RB 4 from four on, chunks of RB
    nrb = lambda c: -(-c.Co // 16)
    assert nrb(B['rb4/nb2']) == 4 and nrb(B['rb4_ragged/nb3']) == 5 and B['rb4_ragged/nb3'].Co % 16 == 8 and nrb(B['rb2_k1/nb2']) == 2
    assert B['rb4_back/nb2'].K == 648 and -(-648 // 32) == 21 and 32 % 9 != 0
    assert B['m257/nb1'].M == 257 and B['rb4/nb3'].M % 2 == 1


def test_k1_pad2_has_outputs_that_are_the_bias_alone():
    c = C.BY_NAME['k1_pad2']
    inp = C.inputs(c)
    y = C.reference(c, inp)[0]
    assert torch.equal(y[:, :, 0, :], inp['bias'].double()[:, None, None].expand(-1, c.NB, c.OW))
    assert torch.equal(y[:, :, :, 0], inp['bias'].double()[:, None, None].expand(-1, c.NB, c.OH))


def test_a_sessions_report_keeps_every_modules_keys(tmp_path, monkeypatch):
    """parity_harness.Harness.finish: the modules of one session share a report file.  Those collected before the module that starts the file afresh
    (merge False: test_gpu_layer_parity.py, behind the depthwise and grouped files in name order) keep their keys; a file left by an EARLIER session is
    still replaced by that module when it comes first."""
    import json

    import parity_harness as H
    path = tmp_path / 'report.json'
    monkeypatch.setenv('XFR_TEST_REPORT', str(path))
    path.write_text(json.dumps({'stale': [1.0, 2.0]}))

    def module(key, merge):
        h = H.Harness()
        h.report[key] = (1e-7, 2e-7)
        h.finish('XFR_TEST_REPORT', merge=merge)
        return json.loads(path.read_text())

    assert sorted(module('layer', False)) == ['layer']                                  # first of the session: the earlier session's file goes
    assert sorted(module('strided', True)) == ['layer', 'strided']
    H._written.discard(str(path))
    path.write_text(json.dumps({'stale': [1.0, 2.0]}))
    assert sorted(module('direct', True)) == ['direct', 'stale']                        # (merge True has always kept what it found)
    assert sorted(module('layer', False)) == ['direct', 'layer', 'stale']               # ... and the afresh module keeps what this session wrote
    assert module('direct', True)['direct'] == [1e-7, 2e-7]


def _layer_gradient(L, NB, dy, w):
    """torch autograd's input gradient of the forward layer L at the output gradient dy [NB][G Co][OH][OW], float64."""
    x = torch.randn((NB, L['G'] * L['Ci'], L['H'], L['W']), dtype=torch.float64, generator=torch.Generator().manual_seed(3), requires_grad=True)
    y = F.conv2d(x, w.double(), None, stride=L['s'], padding=L['p'], groups=L['G'])
    assert tuple(y.shape) == tuple(dy.shape), (tuple(y.shape), tuple(dy.shape))
    return torch.autograd.grad(y, x, dy)[0]


@pytest.mark.parametrize('name', [c.name for c in C.CASES if c.role == 'bwd'])
def test_backward_role_launches_are_autograd_input_gradients(name):
    c = C.BY_NAME[name]
    inp = C.inputs(c)
    wl = C.layer_weight(c)
    assert torch.equal(inp['w'], C.prepared_weight(wl, c.G))
    got = C.conv(c, inp['x'], inp['w'], None, torch.float64).permute(1, 0, 2, 3)
    dy = inp['x'][:, :c.NB].permute(1, 0, 2, 3).double()
    want = _layer_gradient(c.layer, c.NB, dy.clamp(min=0) if c.relu_in else dy, wl)
    assert tuple(got.shape) == tuple(want.shape) and _rel(got, want) <= 1e-12, _rel(got, want)


@pytest.mark.parametrize('name', [c.name for c in C.CASES if c.role == 'phase'])
def test_phase_launches_add_up_to_the_autograd_input_gradient(name):
    """Every phase of the case's layer as a launch of the debug entry, through the reference onto one zero-filled target; the case itself is one of them."""
    c = C.BY_NAME[name]
    L = c.layer
    wl = C.layer_weight(c)
    x = C.inputs(c)['x']
    phases = C.phase_geometry(L['H'], L['W'], L['k'], L['s'], L['p'])
    assert len(phases) == 4 and c.phase in [(q['r'], q['c']) for q in phases]
    target = torch.zeros((c.cout, c.NB) + tuple(c.target), dtype=torch.float64)
    for q in phases:
        pc = C.phase_case('%s/%d%d' % (name, q['r'], q['c']), L, c.NB, q['r'], q['c'], (0, 0), '')
        w = C.prepared_weight(wl, c.G, L['s'], q['r'], q['c'])
        if (q['r'], q['c']) == c.phase:
            assert torch.equal(w, C.inputs(c)['w']) and (pc.OH, pc.OW, pc.origin, pc.pad, pc.pad_dw) == (c.OH, c.OW, c.origin, c.pad, c.pad_dw)
        v = C.live_view(pc, target)
        v.copy_(v + C.conv(pc, x, w, None, torch.float64))
    want = _layer_gradient(L, c.NB, x[:, :c.NB].permute(1, 0, 2, 3).double(), wl)
    got = target.permute(1, 0, 2, 3)
    assert tuple(got.shape) == tuple(want.shape) and _rel(got, want) <= 1e-12, _rel(got, want)
