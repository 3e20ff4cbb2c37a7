"""CPU: the encoder LSTM's launch plan (csrc/lstm.hip: plan_fwd / plan_bwd and the instance table).

A. The six shape queries answer exactly what tests/golden/lstm_plan_queries.npz recorded (tools/gen_lstm_plan_golden.py, run on
   the build before the plan existed) for every shape of the grid, with each fallback switch unset and set.
B. The plan's printable form (las_lstm_plan_describe) is consistent with those queries for every shape: status, kernel family,
   ring fill within the workspace the size query asks for, LDS, block and grid limits, residency, fused input.
Without a GPU the library sizes its geometry for 256 CUs; the switches are read on every call."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SWITCHES = ('none', 'LAS_LSTM_NO_XL', 'LAS_LSTM_NO_GR', 'LAS_LSTM_NO_X32')
QUERIES = ('las_lstm_hx_bytes', 'las_lstm_bwd_ws_bytes', 'las_lstm_bwd_is_ksplit', 'las_lstm_fwd_variant', 'las_lstm_resident_wgs')
HX, WS, KSPLIT, VARIANT, WGS = range(5)
# the int codes of las_lstm_fwd_variant / las_lstm_bwd_is_ksplit (the f32w kernels report as the family they stand in for)
FWD_CODE = {'lstm_fwd_kernel': 0, 'lstm_fwd_f32w_kernel': 0, 'lstm_fwd_gr_kernel': 1, 'lstm_fwd_x32_kernel': 2}
BWD_CODE = {'lstm_bwd_kernel': 0, 'lstm_bwd_ks_kernel': 1, 'lstm_bwd_f32w_kernel': 1, 'lstm_bwd_gr_kernel': 2, 'lstm_bwd_x32_kernel': 3}
LINE = re.compile(r'^(\S+) grid=(\d+) block=(\d+) lds=(\d+) fill=(\d+) ws=(\d+) twin=([01])$')
selected = set()          # table rows some shape of the grid selected, over all switch settings
swept = set()             # ... the settings swept so far


@pytest.fixture(scope='module')
def L():
    m = importlib.import_module('end-to-end-asr-pytorch_amd')
    m.build()
    return m._lib.lib()


@pytest.fixture(scope='module')
def golden():
    with np.load(os.path.join(HERE, 'golden', 'lstm_plan_queries.npz')) as z:
        return {k: z[k] for k in z.files}


def _switch(monkeypatch, sw):
    for s in SWITCHES[1:]:
        monkeypatch.delenv(s, raising=False)
    if sw != 'none':
        monkeypatch.setenv(sw, '1')


def test_golden_grid_is_the_whole_grid(golden):
    """A shrunken grid cannot pass silently: the values the grid was specified with are all there, fully crossed, and with no
    switch set it reaches every variant code, fused input yes and no, and unsupported shapes."""
    sh = golden['shapes']
    want = [{0, 1}, {20, 1200}, {1, 6, 8, 12, 16, 17, 24, 30, 32, 33, 40, 48, 64, 65, 100, 130, 200, 300},
            {16, 40, 64, 160, 256, 320, 500, 512, 514, 640, 768, 1024, 1026, 2048}, {1, 2}]
    n = 1
    for col, vals in enumerate(want):
        have = set(int(v) for v in sh[:, col])
        assert vals <= have, (col, vals - have)
        n *= len(have)
    assert any(int(h) % 2 for h in sh[:, 3]), 'no odd H'
    assert len(set(map(tuple, sh.tolist()))) == len(sh) == n, 'the grid is not the full cross product'
    assert set(golden['fx_I'].tolist()) >= {0, 4, 80, 82, 96, 100}
    g = golden['none']
    assert set(g[:, VARIANT].tolist()) == {0, 1, 2} and set(g[:, KSPLIT].tolist()) == {0, 1, 2, 3}
    assert set(g[:, len(QUERIES):].ravel().tolist()) == {0, 1}
    assert (g[:, WS] == 0).any() and (g[:, WS] > 0).any()


def _describe(L, buf, prec, T, B, H, ND, I, backward):
    rc = L.las_lstm_plan_describe(prec, T, B, H, ND, 1, 0, I, backward, buf, ctypes.c_size_t(len(buf)))
    m = LINE.match(buf.value.decode())
    assert m, buf.value
    name = m.group(1)
    assert (rc == 0) == (name != '-'), (rc, name)
    return (rc, name) + tuple(int(v) for v in m.groups()[1:])


@pytest.mark.parametrize('sw', SWITCHES)
def test_queries_equal_golden_and_plan_is_consistent(L, golden, monkeypatch, sw):
    _sweep(L, golden, monkeypatch, sw)


def _sweep(L, golden, monkeypatch, sw):
    _switch(monkeypatch, sw)
    fx_I = [int(i) for i in golden['fx_I']]
    fns = [getattr(L, q) for q in QUERIES]
    buf = ctypes.create_string_buffer(256)
    want = golden[sw]
    for r, (prec, T, B, H, ND) in enumerate(golden['shapes'].tolist()):
        shape = (sw, prec, T, B, H, ND)
        # A: the six queries
        got = [int(fn(prec, T, B, H, ND)) for fn in fns] + [int(L.las_lstm_fwd_fx_ok(prec, T, B, H, ND, i)) for i in fx_I]
        assert got == want[r].tolist(), (shape, got, want[r].tolist())
        # B, forward
        rc, name, grid, block, lds, fill, ws, twin = _describe(L, buf, prec, T, B, H, ND, 0, 0)
        assert ws == got[HX], shape
        if rc == 0:
            selected.add(name)
            fam = name.split('<')[0]
            assert FWD_CODE[fam] == got[VARIANT], (shape, name)
            assert fill <= got[HX] and 0 < lds <= 160 * 1024 and 0 < grid <= 256, (shape, name, fill, lds, grid)
            # __launch_bounds__: 512 for the 32-unit kernels, 320 for the granule kernel and for lstm_fwd_kernel up to KS = 16, else 256
            ks = int(name.rstrip('>').split(',')[2]) if fam == 'lstm_fwd_kernel' else 0
            bound = 512 if fam == 'lstm_fwd_x32_kernel' else 320 if fam == 'lstm_fwd_gr_kernel' or (fam == 'lstm_fwd_kernel' and ks <= 16) else 256
            assert block in (256, 320, 512) and block <= bound, (shape, name, block)
            assert twin == (fam in ('lstm_fwd_gr_kernel', 'lstm_fwd_x32_kernel')), (shape, name)
        else:
            # (las_lstm_hx_bytes answers for refused shapes too, as it always has, unless the arguments themselves are rejected)
            assert got[VARIANT] == 0 and not any(got[len(QUERIES):]), shape
        for c, i in enumerate(fx_I):
            if i > 0:
                rc_i, name_i = _describe(L, buf, prec, T, B, H, ND, i, 0)[:2]
                assert (rc_i == 0) == (got[len(QUERIES) + c] == 1), (shape, i, rc_i)
                if rc_i == 0:
                    selected.add(name_i)
                    assert rc == 0 and name_i.endswith(',true>') and name_i.split('<')[0] in ('lstm_fwd_gr_kernel', 'lstm_fwd_x32_kernel'), (shape, i, name_i)
            else:
                assert got[len(QUERIES) + c] == 0, shape
        # B, backward
        rc, name, grid, block, lds, fill, ws, twin = _describe(L, buf, prec, T, B, H, ND, 0, 1)
        assert (rc == 0) == (got[WS] > 0), (shape, rc, got[WS])
        if rc == 0:
            selected.add(name)
            fam = name.split('<')[0]
            assert BWD_CODE[fam] == got[KSPLIT] and ws == got[WS], (shape, name)
            assert fill <= got[WS] and 0 < lds <= 160 * 1024 and 0 < grid <= 256, (shape, name, fill, lds, grid)
            bound = 512 if fam == 'lstm_bwd_x32_kernel' else 320 if fam == 'lstm_bwd_gr_kernel' else 256
            assert block in (256, 320, 512) and block <= bound, (shape, name, block)
            assert 0 < got[WGS] <= grid, (shape, got[WGS], grid)
            assert twin == (fam in ('lstm_bwd_gr_kernel', 'lstm_bwd_x32_kernel')), (shape, name)
        else:
            assert got[KSPLIT] == 0 and got[WS] == 0, shape
    swept.add(sw)


def test_every_family_is_selected(L, golden, monkeypatch):
    """Reports the table rows no grid shape selects under any switch setting; each of the nine families must be selected."""
    for sw in SWITCHES:
        if sw not in swept:              # (run on its own: the sweeps above have not filled `selected`)
            _sweep(L, golden, monkeypatch, sw)
    src = open(os.path.join(os.path.dirname(HERE), 'end-to-end-asr-pytorch_amd', 'csrc', 'lstm.hip')).read()
    rows = {f'{k}<{a}>' for k, a in re.findall(r'\bROW\((lstm_\w+), ([^()\s]+)\)', src)}
    assert len(rows) >= 60 and selected <= rows, selected - rows
    print('table rows no shape of the grid selects:', sorted(rows - selected))
    assert {r.split('<')[0] for r in selected} == set(FWD_CODE) | set(BWD_CODE)
