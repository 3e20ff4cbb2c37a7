"""GPU parity of the fp32-mode (Bi)LSTM recurrence and BPTT at hidden sizes whose f32 W_hh slab does not fit LDS
(lstm_fwd_f32w_kernel / lstm_bwd_f32w_kernel: weight fragments in registers), H = 512 .. 1024, against the oracle
(torch packed LSTM) at the project's f32 bound -- atol 2e-4 / rtol 1e-3, weight gradients scaled by their largest
entry -- instead of the 8e-2 / 5e-2 of bf16 mode these geometries were judged at before.  fp32 oracle vs an fp64 run of
the same oracle on these shapes: at most 1.3 % of that bound, so a correct fp32 kernel cannot miss it for rounding."""
import importlib
import numpy as np
import pytest
import torch

from test_encoder_gpu import test_lstm_shapes_vs_oracle as lstm_shapes_vs_oracle, cat_lstm_weights, close, T_, DEV

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    importlib.import_module('end-to-end-asr-pytorch_amd')
    return importlib.import_module('end-to-end-asr-pytorch_amd.ops')


SHAPES = [(21, 24, 16, 512),
          (13, 24, 32, 1024),
          (7, 24, 4096, 1024),        # C5's concat input
          (9, 40, 16, 1024),          # two batch tiles per slice
          (11, 12, 16, 768),
          (17, 24, 16, 600),          # H not a multiple of 16
          (151, 12, 32, 1024),        # 37 laps of the 4-slot ring
          (120, 40, 16, 512)]


@pytest.mark.parametrize('T,B,Iin,H', SHAPES)
def test_lstm_f32_wide_vs_oracle(ops, T, B, Iin, H):
    """Forward, d x and every weight gradient of one bidirectional layer in f32 mode (status == 0 asserted inside)."""
    lstm_shapes_vs_oracle(ops, T, B, Iin, H, 'f32')


def test_lstm_f32_wide_no_xl(ops, monkeypatch):
    """H = 512 takes the XCD-grouped launch (L2-local hand-off) by default; the same shape through the cross-XCD sc1
    protocol.  (H = 1024 groups span two XCDs and always take the latter.)"""
    monkeypatch.setenv('LAS_LSTM_NO_XL', '1')
    lstm_shapes_vs_oracle(ops, 21, 24, 16, 512, 'f32')


@pytest.mark.parametrize('style,bidir', [('concat', True), ('drop', True), ('concat', False)])
def test_lstm_layer_f32_wide_subsampled(ops, style, bidir):
    """ops.lstm_layer at H = 1024 with sr = 2 (concat and drop output addressing) and a unidirectional layer, ragged
    lengths, against oracle.las_ref.rnn_layer."""
    from oracle import las_ref as R
    T, B, Iin, H, sr = 14, 12, 24, 1024, 2
    rng = np.random.RandomState(77)
    lens = sorted(rng.randint(T // 3, T + 1, size=B).tolist(), reverse=True); lens[0] = T
    x = np.zeros((B, T, Iin), np.float32)
    for b, l in enumerate(lens):
        x[b, :l] = rng.randn(l, Iin)
    W = {}
    for sfx in (['', '_reverse'] if bidir else ['']):
        W['L.layer.weight_ih_l0' + sfx] = torch.tensor((rng.randn(4 * H, Iin) / np.sqrt(Iin)).astype(np.float32), requires_grad=True)
        W['L.layer.weight_hh_l0' + sfx] = torch.tensor((rng.randn(4 * H, H) / np.sqrt(H)).astype(np.float32), requires_grad=True)
        W['L.layer.bias_ih_l0' + sfx] = torch.tensor((0.1 * rng.randn(4 * H)).astype(np.float32), requires_grad=True)
        W['L.layer.bias_hh_l0' + sfx] = torch.tensor((0.1 * rng.randn(4 * H)).astype(np.float32), requires_grad=True)
    xr = torch.tensor(x, requires_grad=True)
    yr, _ = R.rnn_layer(xr, lens, W, 'L', sr, style, bidir, fast=True)
    gy = rng.randn(*yr.shape).astype(np.float32)
    (yr * torch.tensor(gy)).sum().backward()
    dd = {k[len('L.layer.'):]: v.detach().numpy() for k, v in W.items()}
    gd = {k[len('L.layer.'):]: v.grad.numpy() for k, v in W.items()}
    w_ih, w_hh, b_ih, b_hh = [T_(v, True) for v in cat_lstm_weights(dd, '', bidir)]
    xg = T_(x, True)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.set_precision('f32')
    try:
        y = ops.Transpose01Fn.apply(ops.lstm_layer(ops.Transpose01Fn.apply(xg), torch.tensor(lens, dtype=torch.int32, device=DEV),
                                                   w_ih, w_hh, b_ih, b_hh, sr, style == 'concat', status))
        (y * T_(gy)).sum().backward()
        ops.join_side_stream()
        torch.cuda.synchronize()
    finally:
        ops.set_precision('bf16')
    assert int(status.item()) == 0
    tol = dict(atol=2e-4, rtol=1e-3)
    assert tuple(y.shape) == tuple(yr.shape)
    close(y, yr.detach().numpy(), tol)
    close(xg.grad, xr.grad.numpy(), tol)
    g_ih, g_hh, g_bi, g_bh = cat_lstm_weights(gd, '', bidir)
    scale = max(1.0, np.abs(g_hh).max(), np.abs(g_ih).max())
    close(w_ih.grad / scale, g_ih / scale, tol)
    close(w_hh.grad / scale, g_hh / scale, tol)
    close(b_ih.grad / scale, g_bi / scale, tol)
    close(b_hh.grad / scale, g_bh / scale, tol)
