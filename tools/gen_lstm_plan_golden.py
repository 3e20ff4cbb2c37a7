"""Record what the encoder LSTM's six shape queries answer over a grid of shapes, as tests/golden/lstm_plan_queries.npz.

    python tools/gen_lstm_plan_golden.py [out.npz]

Needs no GPU (without one the queries answer for 256 CUs) and calls only las_lstm_hx_bytes, las_lstm_bwd_ws_bytes,
las_lstm_bwd_is_ksplit, las_lstm_fwd_variant, las_lstm_resident_wgs and las_lstm_fwd_fx_ok, so it runs against any build
that has them: run it in a checkout of the commit whose answers are to be pinned, then tests/test_lstm_plan_cpu.py holds
every later build to them.  Arrays: shapes [N][5] = prec, T, B, H, ND; fx_I [6]; one [N][5 + 6] array per switch setting,
columns in the order above, las_lstm_fwd_fx_ok once per fx_I value."""
import importlib
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PRECS = (0, 1)                                # LAS_PREC_BF16, LAS_PREC_F32
HS = (16, 40, 64, 160, 256, 320, 500, 512, 514, 640, 768, 1024, 1026, 2048, 255)
BS = (1, 6, 8, 12, 16, 17, 24, 30, 32, 33, 40, 48, 64, 65, 100, 130, 200, 300)
NDS = (1, 2)
TS = (20, 1200)                               # 1200 crosses the 2^31-byte rule at large B * H
FX_I = (0, 4, 80, 82, 96, 100)
SWITCHES = ('none', 'LAS_LSTM_NO_XL', 'LAS_LSTM_NO_GR', 'LAS_LSTM_NO_X32')
QUERIES = ('las_lstm_hx_bytes', 'las_lstm_bwd_ws_bytes', 'las_lstm_bwd_is_ksplit', 'las_lstm_fwd_variant', 'las_lstm_resident_wgs')


def answers(L, shapes, fx_i):
    out = np.zeros((len(shapes), len(QUERIES) + len(fx_i)), np.int64)
    fns = [getattr(L, q) for q in QUERIES]
    for r, (prec, T, B, H, ND) in enumerate(shapes):
        for c, fn in enumerate(fns):
            out[r, c] = fn(prec, T, B, H, ND)
        for c, i in enumerate(fx_i):
            out[r, len(fns) + c] = L.las_lstm_fwd_fx_ok(prec, T, B, H, ND, i)
    return out


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'tests', 'golden', 'lstm_plan_queries.npz')
    L = importlib.import_module('end-to-end-asr-pytorch_amd')._lib.lib()
    shapes = [tuple(int(v) for v in s) for s in itertools.product(PRECS, TS, BS, HS, NDS)]
    arrays = dict(shapes=np.array(shapes, np.int32), fx_I=np.array(FX_I, np.int32))
    for sw in SWITCHES:
        for other in SWITCHES[1:]:
            os.environ.pop(other, None)
        if sw != 'none':
            os.environ[sw] = '1'
        arrays[sw] = answers(L, shapes, FX_I)
        os.environ.pop(sw, None)
    np.savez_compressed(out, **arrays)
    print(f'{out}: {len(shapes)} shapes x {len(SWITCHES)} switch settings, {os.path.getsize(out)} bytes')


if __name__ == '__main__':
    main()
